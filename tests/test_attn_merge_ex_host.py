"""cfx_attn_merge_ex (the ring-attention block merge for fp16 or bf16 blocks, the layer's final cast in the launch) - everything that can
be checked without a GPU: the symbol, its argument errors, the compiled kernels' resource rows, and that CPU tensors keep the eager
formula."""
import json
import os
import re
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BSHD, FIRST, BF = 1, 2, 0x100


def test_the_symbol_is_declared_exported_and_bound():
    from compactfusion_amd import _lib
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "cfx.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+cfx_attn_merge_ex\s*\(", hdr)
    for name, val in (("CFX_MERGE_BSHD", 1), ("CFX_MERGE_FIRST", 2), ("CFX_ELEM_BF16", 0x100), ("CFX_ABI_VERSION", 2)):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, hex(val) if val > 9 else val), hdr), name
    assert hasattr(lib, "cfx_attn_merge_ex")
    bound = {n: a for n, _, a in _lib.SYMBOLS}
    assert len(bound["cfx_attn_merge_ex"]) == 14
    assert (_lib.MERGE_BSHD, _lib.MERGE_FIRST, _lib.ELEM_BF16) == (BSHD, FIRST, BF)
    assert lib.cfx_abi_version() == 2
    # the two existing merge calls are still there, as they were
    assert len(bound["cfx_attn_merge"]) == 12 and len(bound["cfx_attn_merge_wait"]) == 14


def test_argument_errors_come_in_the_stated_order():
    """NULL -1, unknown flag bit -4, shape -2, alignment -3 - each case has every LATER fault too, so the order is what is tested.
    (A context created without a GPU: nothing here reaches a launch.)"""
    from compactfusion_amd import _lib
    lib = _lib.load()
    ctx = lib.cfx_create(0)
    assert ctx
    out, lse, bo, bl, fin = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    B, S, H, D = 1, 4, 2, 64

    def call(out=out, lse=lse, bo=bo, bl=bl, D=D, flags=BSHD, fin=None, c=ctx):
        return lib.cfx_attn_merge_ex(c, out, lse, bo, bl, B, S, H, D, flags, None, 0, fin, None)
    assert call(c=None) == -1
    for elem in (0, BF):
        # NULL first: in front of a bad flag, a bad shape and a misaligned pointer
        assert call(lse=None, flags=elem | 0x8, D=20, bo=bo + 2) == -1
        assert call(bo=None, flags=elem | 0x8, D=20) == -1
        assert call(bl=None, flags=elem | BSHD, D=20) == -1
        assert b"null" in lib.cfx_last_error_string(ctx)
        # out may be NULL only with FIRST and final_out together
        assert call(out=None, flags=elem | BSHD) == -1
        assert call(out=None, flags=elem | BSHD | FIRST) == -1
        assert call(out=None, flags=elem | BSHD, fin=fin) == -1
        # an unknown flag bit: in front of the shape and the alignment
        for bad in (0x4, 0x8, 0x200, 0x1000, 0x10000, 0x40000000):
            assert call(flags=elem | bad, D=20, bo=bo + 2) == -4, hex(bad)
            assert call(flags=elem | BSHD | FIRST | bad) == -4, hex(bad)
        assert b"flag" in lib.cfx_last_error_string(ctx)
        assert call(flags=-1) == -4
        # the shape: in front of the alignment
        for d in (0, -8, 20, 4, 520, 1024):
            assert call(flags=elem | BSHD, D=d, bo=bo + 2, fin=fin + 4) == -2, d
        # 16-byte alignment of out, block_out and final_out
        assert call(flags=elem, out=out + 4) == -3
        assert call(flags=elem, bo=bo + 2) == -3
        assert call(flags=elem | BSHD, fin=fin + 8) == -3
        assert call(flags=elem | BSHD | FIRST, out=None, fin=fin + 2) == -3
        assert b"aligned" in lib.cfx_last_error_string(ctx)
    lib.cfx_destroy(ctx)


@pytest.fixture(scope="module")
def rows():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import resource_usage
    return resource_usage.collect()


def test_the_new_kernel_has_four_forms_without_scratch_and_k_attn_merge_is_the_parents(rows):
    ex = {k["demangled"]: k for k in rows if k["demangled"].startswith("k_attn_merge_ex<")}
    assert sorted(ex) == sorted(f"k_attn_merge_ex<{e}, {f}>" for e in ("ElemF16", "ElemBF16") for f in ("false", "true")), sorted(ex)
    for k in ex.values():
        assert k["file"] == "cfx_api.hip" and k.get("scratch", 0) == 0 and k.get("lds", 0) == 0, k
        assert k["vgpr"] + k.get("agpr", 0) <= 64, k              # a streaming kernel: eight waves a SIMD, like k_attn_merge
    parent = json.load(open(os.path.join(REPO, "tests", "golden", "resource_rows_parent.json")))
    want = [p for p in parent if p["demangled"].startswith("_Z12k_attn_merge")]
    assert len(want) == 1 and want[0]["demangled"] == "_Z12k_attn_mergePfS_PKDF16_PKfiiiiimmmiPKjjPjx"
    got = [k for k in rows if k["name"] == want[0]["demangled"]]
    assert len(got) == 1, "k_attn_merge changed its mangled name"
    assert {f: got[0].get(f, 0) for f in ("vgpr", "agpr", "sgpr", "lds", "scratch")} == {f: want[0][f] for f in ("vgpr", "agpr", "sgpr", "lds", "scratch")}
    assert got[0]["file"] == want[0]["file"]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_cpu_tensors_keep_the_eager_formula(monkeypatch, dtype):
    import torch.nn.functional as F
    from compactfusion_amd.compact import attention as A
    tried = []
    monkeypatch.setattr(A, "_merge_native", lambda *a: tried.append(a))
    g = torch.Generator().manual_seed(2)
    B, S, H, D = 2, 9, 3, 64
    out = lse = ref_o = ref_l = None
    for blk in range(3):
        bo = torch.randn(B, S, H, D, generator=g).to(dtype)
        bl = torch.randn(B, H, S, generator=g)
        out, lse = A.update_out_and_lse(out, lse, bo, bl)
        bo32, bl4 = bo.to(torch.float32), bl.transpose(-2, -1).unsqueeze(-1)
        if ref_o is None:
            ref_o, ref_l = bo32, bl4
        else:
            ref_o = ref_o - torch.sigmoid(bl4 - ref_l) * (ref_o - bo32)
            ref_l = ref_l - F.logsigmoid(ref_l - bl4)
    assert not tried, "the native merge was attempted on CPU tensors"
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, S, H, D) and tuple(lse.shape) == (B, S, H, 1)
    assert torch.equal(out, ref_o) and torch.equal(lse, ref_l)
