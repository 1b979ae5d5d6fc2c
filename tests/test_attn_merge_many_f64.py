"""The one-launch merge of all of a layer's attention blocks (cfx_attn_merge_many, merge_blocks, configure(attn_merge=...)) on the CPU: the
float64 witness and derived bound of tests/_merge_many_f64.py against the chain's float64 result and against a numpy fp32 transcription
of the kernel; planted errors; the eager fallback; the C-ABI's argument checks; the new source's resource rows; the setting; and the
calls `_blocks` makes in either mode.  No GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _merge_f64 as M
import _merge_many_f64 as N

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c["id"] for c in M.CASES]
SMALL = [c for c in M.CASES if c["shape"] != M.FLUX]


@pytest.mark.parametrize("case", M.CASES, ids=IDS)
def test_witness_equals_the_chain_in_float64(case):
    """the direct formula and the chain are the same function: 1e-12 relative (out: of the largest block value at the element, the
    scale of a convex combination; lse: of max(1, |lse|))"""
    blocks = M.build(case)
    o, l = N.witness(blocks)[:2]
    ro, rl = M.reference_and_bound(blocks)[:2]
    scale = np.max(np.stack([np.abs(b[0].astype(np.float64)) for b in blocks]), axis=0)
    assert (np.abs(o - ro) <= 1e-12 * scale).all(), float(np.max(np.abs(o - ro) / np.maximum(scale, 1e-300)))
    assert (np.abs(l - rl) <= 1e-12 * np.maximum(1.0, np.abs(rl))).all()


@pytest.mark.parametrize("case", M.CASES, ids=IDS)
def test_transcription_meets_the_bound(case):
    blocks = M.build(case)
    for err in (0.0, 1.0, -1.0):
        o, l = N.kernel_fp32(blocks, exp_err=err)
        fo, fl = N.check(o, l, blocks, f"k_attn_merge_many in numpy fp32, exponentials off by {err:+.0f} x their stated error")
        print(f"{case['id']}: transcription ({err:+.0f}) {fo:.3f} / {fl:.3f} of the bound (out / lse)")


@pytest.mark.parametrize("case", SMALL[::5], ids=IDS[:len(SMALL):5])
def test_a_single_block_is_exact(case):
    blocks = M.build(case)[:1]
    for err in (0.0, 1.0, -1.0):
        o, l = N.kernel_fp32(blocks, exp_err=err)
        assert np.array_equal(o, blocks[0][0]) and np.array_equal(l, blocks[0][1])
        assert N.check(o, l, blocks) == (0.0, 0.0)
    with pytest.raises(AssertionError):                       # ... and the check holds a single block to equality, not to a bound
        N.check(np.nextafter(blocks[0][0], np.float32(np.inf)), blocks[0][1], blocks)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("plant", N.PLANTS)
def test_planted_errors_exceed_the_bound(plant, dtype):
    caught = []
    for c in SMALL:
        if c["dtype"] != dtype or (plant == "nomax" and c["offset"] == 0.0):
            continue
        blocks = M.build(c)
        o, l = N.kernel_fp32(blocks, plant=plant)
        try:
            N.check(o, l, blocks)
        except AssertionError:
            caught.append(c["id"])
    assert caught, f"{plant} passes the check on every {dtype} case"
    if plant == "nomax":                                      # every case at offset +-300 shows it
        assert len(caught) == sum(1 for c in SMALL if c["dtype"] == dtype and c["offset"] != 0.0)


@pytest.mark.parametrize("case", M.CASES, ids=IDS)
def test_eager_fallback_on_cpu_tensors(case, monkeypatch):
    from compactfusion_amd.compact import attention as A
    monkeypatch.setattr(A, "_merge_many_native", lambda *a: pytest.fail("CPU tensors reached the native launch"))
    blocks = M.build(case)
    tdt = torch.float16 if case["dtype"] == "fp16" else torch.bfloat16
    outs = [torch.from_numpy(o).to(tdt) for o, _ in blocks]
    lses = [torch.from_numpy(l).permute(0, 2, 1).contiguous() for _, l in blocks]            # (B, H, S), as block_attention returns it
    out, lse = A.merge_blocks(outs, lses)
    assert out.dtype == torch.float32 and out.shape == blocks[0][0].shape and lse.shape == blocks[0][1].shape + (1,) and lse.dtype == torch.float32
    fo, fl = N.check(out.numpy(), lse.squeeze(-1).numpy(), blocks, "merge_blocks, eager fallback")
    print(f"{case['id']}: eager fallback {fo:.3f} / {fl:.3f} of the bound")
    if case["shape"] != M.FLUX:
        o16, l2 = A.merge_blocks(outs, lses, tdt)
        assert o16.dtype == tdt and torch.equal(o16, out.to(tdt)) and torch.equal(l2, lse)
        one, lone = A.merge_blocks(outs[:1], lses[:1], tdt)
        assert torch.equal(one, outs[0]) and np.array_equal(lone.squeeze(-1).numpy(), blocks[0][1])
    with pytest.raises(ValueError):
        A.merge_blocks([], [])


def test_c_abi_argument_checks_without_a_gpu():
    """every argument error, in the documented order: NULL, flag bits, n / shape, alignment (a pending gate error needs a device)"""
    from compactfusion_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(REPO, "include", "cfx.h")).read()
    assert re.search(r"\bint cfx_attn_merge_many\(cfx_ctx\* ctx, int n, const void\* const\* block_outs", hdr)
    assert "#define CFX_MERGE_MAX_BLOCKS 16" in hdr and "#define CFX_MERGE_OUT_F32 4" in hdr
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT cfx_attn_merge_many\b", exported)
    assert "cfx_attn_merge_many" in {n for n, _, _ in _lib.SYMBOLS} and hasattr(lib, "cfx_attn_merge_many")
    assert _lib.MERGE_OUT_F32 == 4 and _lib.MERGE_MAX_BLOCKS == 16 and lib.cfx_abi_version() == 2
    ctx = lib.cfx_create(0)
    assert ctx
    f = lib.cfx_attn_merge_many
    P = ctypes.c_void_p * 17
    bo = P(*[0x10000 + 0x1000 * i for i in range(17)])
    bl = P(*[0x40000 + 0x1000 * i for i in range(17)])
    out, lse = 0x80000, 0x90000
    NULL, SHAPE, ALIGN, CODEC = -1, -2, -3, -4
    # 1. NULL pointers, table entries included - before anything else
    assert f(None, 2, bo, bl, 1, 4, 2, 64, 0, out, lse, None) == NULL
    assert f(ctx, 2, None, bl, 1, 4, 2, 64, 0, out, lse, None) == NULL
    assert f(ctx, 2, bo, None, 1, 4, 2, 64, 0, out, lse, None) == NULL
    assert f(ctx, 2, bo, bl, 1, 4, 2, 64, 0, None, lse, None) == NULL
    assert f(ctx, 2, bo, bl, 1, 4, 2, 64, 0, out, None, None) == NULL
    assert b"null" in lib.cfx_last_error_string(ctx)
    for k in (0, 1, 15):
        holed = P(*[None if i == k else 0x10000 + 0x1000 * i for i in range(17)])
        assert f(ctx, 16, holed, bl, 1, 4, 2, 64, 0, out, lse, None) == NULL
        assert f(ctx, 16, bo, holed, 1, 4, 2, 64, 0, out, lse, None) == NULL
        assert f(ctx, 16, holed, bl, 1, 4, 2, 20, 0x40, 0x80002, lse, None) == NULL          # ... whatever else is wrong
    holed = P(*[None if i == 3 else 0x10000 + 0x1000 * i for i in range(17)])
    assert f(ctx, 3, holed, bl, 1, 4, 2, 64, 0x40, out, lse, None) == CODEC                      # (entry 3 is not one of 3 blocks)
    # 2. flag bits: BSHD, BF16 and OUT_F32 only - CFX_MERGE_FIRST is refused
    for bad in (_lib.MERGE_FIRST, 8, 0x40, 0x200, _lib.MERGE_BSHD | _lib.MERGE_FIRST, -1):
        assert f(ctx, 2, bo, bl, 1, 4, 2, 64, bad, out, lse, None) == CODEC, bad
        assert f(ctx, 0, bo, bl, 1, 4, 2, 20, bad, 0x80002, lse, None) == CODEC                 # ... before n, the shape and the alignment
    assert b"flag" in lib.cfx_last_error_string(ctx)
    # 3. n outside 1 .. 16, the shape rule
    ok_flags = (0, _lib.MERGE_BSHD, _lib.ELEM_BF16, _lib.MERGE_OUT_F32, _lib.MERGE_BSHD | _lib.ELEM_BF16 | _lib.MERGE_OUT_F32)
    for fl in ok_flags:
        for n in (0, 17, -1, 1 << 20):
            assert f(ctx, n, bo, bl, 1, 4, 2, 64, fl, 0x80002, lse, None) == SHAPE, (fl, n)
        for B, S, H, D in ((1, 4, 2, 20), (1, 4, 2, 520), (1, 4, 2, 0), (0, 4, 2, 64), (1, 0, 2, 64), (1, 4, 0, 64), (1, 4, 2, -8)):
            assert f(ctx, 2, bo, bl, B, S, H, D, fl, 0x80002, lse, None) == SHAPE, (B, S, H, D)
    # 4. 16-byte alignment of out and of every block_out (the lse tensors are fp32: 4 bytes)
    assert f(ctx, 2, bo, bl, 1, 4, 2, 64, 0, 0x80008, lse, None) == ALIGN
    for k in (0, 7, 15):
        off = P(*[0x10000 + 0x1000 * i + (2 if i == k else 0) for i in range(17)])
        assert f(ctx, 16, off, bl, 1, 4, 2, 64, _lib.MERGE_OUT_F32, out, lse, None) == ALIGN
    lib.cfx_destroy(ctx)


def test_resource_rows_of_the_new_source():
    """cfx_merge.hip alone: exactly the four k_attn_merge_many instantiations plus the k_copy_probe cfx_device.h puts in every
    translation unit; no scratch, no LDS, at most 128 VGPRs.  The source sits in a list of its own, beside SRC and CAPTURE_SRC."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import resource_usage as RU
    finally:
        sys.path.pop(0)
    from compactfusion_amd import build as B
    assert [os.path.basename(p) for p in B.MERGE_SRC] == ["cfx_merge.hip"]
    assert not set(B.MERGE_SRC) & (set(B.SRC) | set(B.CAPTURE_SRC))
    rows = RU._one(B.MERGE_SRC[0])
    names = [re.sub(r"^void ", "", re.sub(r"\(.*$", "", d)) for d in RU.demangle([r["name"] for r in rows])]
    assert sorted(names) == sorted(["k_copy_probe"] + [f"k_attn_merge_many<{e}, {f}>" for e in ("ElemF16", "ElemBF16") for f in ("true", "false")]), names
    for r, name in zip(rows, names):
        assert r.get("scratch", 0) == 0 and r.get("lds", 0) == 0, (name, r)
        assert r.get("vgpr", 0) + r.get("agpr", 0) <= 128, (name, r)
    api = open(os.path.join(B.PKG_DIR, "csrc", "cfx_api.hip")).read()
    assert "merge_many" not in api                            # no kernel template of cfx_api.hip gained an instantiation
    import inspect
    assert "MERGE_SRC" in inspect.getsource(B.needs_build) and "MERGE_SRC" in inspect.getsource(B.build_lib)      # built into, and a dependency of, both libraries


def test_configure_attn_merge(monkeypatch):
    import compactfusion_amd
    from compactfusion_amd import config
    config.reset()
    try:
        monkeypatch.delenv("CFX_ATTN_MERGE", raising=False)
        assert config.get("attn_merge") == "chain" and compactfusion_amd.configure()["attn_merge"] == "chain"
        monkeypatch.setenv("CFX_ATTN_MERGE", "once")
        assert config.get("attn_merge") == "once"
        assert compactfusion_amd.configure(attn_merge="chain")["attn_merge"] == "chain"           # an explicit configure() overrides it
        assert compactfusion_amd.configure(attn_merge="once")["attn_merge"] == "once"
        with pytest.raises(ValueError):
            compactfusion_amd.configure(attn_merge="twice")
        assert config.get("attn_merge") == "once"
        config.reset()
        monkeypatch.setenv("CFX_ATTN_MERGE", "both")
        with pytest.raises(ValueError):
            config.get("attn_merge")
    finally:
        config.reset()
    assert "attn_merge" in config.__doc__ and "CFX_ATTN_MERGE" in config.__doc__
    assert "CFX_ATTN_MERGE" in open(os.path.join(REPO, "INTEGRATION.md")).read()


# ---- _blocks on CPU stand-ins: which calls either mode makes ---------------------------------------------------------------------------
W, SHAPE = 4, (1, 6, 2, 16)


@pytest.fixture
def layer(monkeypatch):
    """a steady layer of W ranks with CPU tensors for its peers' states, and a spy on the merge / wait calls of compact/ring.py"""
    from compactfusion_amd import config
    from compactfusion_amd.compact import attention as A
    from compactfusion_amd.compact import ring as R
    g = torch.Generator().manual_seed(7)
    q, k, v = (torch.randn(SHAPE, generator=g).to(torch.float16) for _ in range(3))
    peers = [(s, torch.randn(SHAPE, generator=g).to(torch.float16), torch.randn(SHAPE, generator=g).to(torch.float16)) for s in range(1, W)]
    st = R._SteadyLayer.__new__(R._SteadyLayer)
    st.world, st._peers, st._fast = W, peers, False
    calls = []

    def spied(name, fn):
        def wrap(*a, **kw):
            calls.append((name, a))
            return fn(*a, **kw)
        return wrap
    monkeypatch.setattr(R, "merge_blocks", spied("merge_blocks", A.merge_blocks))
    monkeypatch.setattr(R, "update_out_and_lse", spied("update_out_and_lse", A.update_out_and_lse))
    monkeypatch.setattr(R, "flag_wait", lambda wait, device: calls.append(("flag_wait", wait)))
    monkeypatch.setattr(A, "flag_wait", lambda wait, device: calls.append(("flag_wait(in merge)", wait)))
    config.reset()
    yield st, q, k, v, peers, calls
    config.reset()


def _eager(q, kvs):
    """softmax attention of q over the concatenated K,V, fp32"""
    k = torch.cat([kk for kk, _ in kvs], dim=1).float().transpose(1, 2)
    v = torch.cat([vv for _, vv in kvs], dim=1).float().transpose(1, 2)
    s = torch.matmul(q.float().transpose(1, 2), k.transpose(-1, -2)) * q.shape[-1] ** -0.5
    return torch.matmul(torch.softmax(s, dim=-1), v).transpose(1, 2), torch.logsumexp(s, dim=-1)


@pytest.mark.parametrize("lane", [False, True])
def test_blocks_once_makes_one_merge_and_w_minus_1_waits(layer, lane):
    import compactfusion_amd
    st, q, k, v, peers, calls = layer
    issued = []
    args = (lambda s, lean: issued.append((s, lean)), lambda r: 0x1000 + 64 * r, 5) if lane else ()
    compactfusion_amd.configure(attn_merge="chain")
    want = st._blocks(q, k, v, q.shape[-1] ** -0.5, None, *args)
    assert [c[0] for c in calls] == (["update_out_and_lse", "flag_wait(in merge)"] * (W - 1) + ["update_out_and_lse"] if lane
                                     else ["update_out_and_lse"] * W), calls                  # today's calls
    chain_issued, chain_waits = list(issued), [c[1] for c in calls if c[0].startswith("flag_wait")]
    del calls[:], issued[:]
    compactfusion_amd.configure(attn_merge="once")
    got = st._blocks(q, k, v, q.shape[-1] ** -0.5, None, *args)
    names = [c[0] for c in calls]
    assert names.count("merge_blocks") == 1 and names[-1] == "merge_blocks" and "update_out_and_lse" not in names, names
    assert names.count("flag_wait") == (W - 1 if lane else 0) and "flag_wait(in merge)" not in names
    merge_args = calls[-1][1]
    assert len(merge_args[0]) == W and len(merge_args[1]) == W and merge_args[2] == q.dtype
    if lane:
        waits = [c[1] for c in calls if c[0] == "flag_wait"]
        assert waits == [(0x1000 + 64 * (s + 1), 5) for s in range(W - 1)] == chain_waits     # the same flags and epoch the chain's merges waited on
        assert issued == chain_issued == [(s, False) for s in range(W)]                       # issue(s, lean) where it always was
    # the same types, shapes and views, and the same attention
    assert got[2] is None and want[2] is None
    for a, b in zip(got[:2], want[:2]):
        assert a.dtype == b.dtype and a.shape == b.shape and a.stride() == b.stride()
    ref_o, ref_l = _eager(q, [(k, v)] + [(kk, vv) for _, kk, vv in peers])
    for res in (got, want):
        assert torch.allclose(res[0].float(), ref_o, atol=2e-3, rtol=2e-3) and torch.allclose(res[1], ref_l, atol=1e-4, rtol=1e-5)
