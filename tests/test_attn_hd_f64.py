"""The native attention forward at the head dims between 64 and 128 (cfx_attn_fwd_blocks_hd, attention_blocks, patch_gather_fwd under
configure(attention="native")) on the CPU: the case list's own conditions; the witness and the bound ARE tests/_attn_var_f64.py's; the
planted errors of tests/_attn_hd_cases.py, each at least 10 x the bound on every case that can show it; CPU tensors never reach a launch;
the C-ABI's argument checks; the new source's resource rows; which calls patch_gather_fwd makes, on stand-ins.  No GPU."""
import ctypes
import inspect
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _attn_f64 as W
import _attn_hd_cases as HC
import _attn_var_cases as VC
import _attn_var_f64 as VW

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
_refs = {}


def ref_of(case, dtype):
    """the case's inputs and its witness / bound, computed once"""
    key = (case["id"], dtype)
    if key not in _refs:
        q, ks, vs, scale = VC.build(case, dtype)
        _refs[key] = (q, ks, vs, scale, VW.reference_and_bound(q, ks, vs, scale, dtype))
    return _refs[key]


def test_case_list_covers_what_it_claims():
    cs = HC.CASES
    ids = [c["id"] for c in cs]
    assert len(set(ids)) == len(cs) and 45 <= len(cs) <= 60
    assert HC.DIMS == (72, 80, 88, 96, 104, 112, 120) and all(c["H"] == 3 for c in cs)
    want = [[1], [65, 64, 63], [100, 37, 128, 5], list(range(1, 17)), [64, 128, 192]]
    for D in HC.DIMS:
        mine = [c for c in cs if c["D"] == D]
        assert [c["sks"] for c in mine if c["kind"] == "gauss"] == want                  # every length list, gaussian, at every D
        assert sum(c["kind"] == "peak" for c in mine) >= 2 and {c["B"] for c in mine} == {1, 2}
    assert {c["Sq"] for c in cs} == {1, 33, 129} and {c["kind"] for c in cs} == {"gauss", "peak", "ramp"}
    assert 2 <= sum(c["kind"] == "ramp" for c in cs) <= 5
    for sks in want:                                                                     # every list with every Sq and both B somewhere
        assert {c["Sq"] for c in cs if c["sks"] == sks and c["kind"] == "gauss"} == {1, 33, 129}
        assert {c["B"] for c in cs if c["sks"] == sks and c["kind"] == "gauss"} == {1, 2}
    for dtype in TDT:
        for c in cs:
            q, ks, vs, scale, _ = ref_of(c, dtype)
            assert q.shape == (c["B"], c["Sq"], 3, c["D"]) and [k.shape for k in ks] == [(c["B"], n, 3, c["D"]) for n in c["sks"]] == [v.shape for v in vs]
            assert scale == float(np.float32(c["D"] ** -0.5))


def test_witness_and_bound_are_the_unequal_length_ones():
    """no new witness, no new bound, no new constant: the objects of tests/_attn_var_f64.py, with the true D"""
    assert HC.W.witness is VW.witness is W.witness and HC.W.scores is VW.scores and VW.check is W.check and VW.excess is W.excess
    assert not [n for n in dir(HC) if n in ("U", "SLACK", "EPS", "SUB", "reference_and_bound", "check", "excess")]
    case = next(c for c in HC.CASES if c["D"] == 72 and c["sks"] == [65, 64, 63] and c["kind"] == "gauss")
    q, ks, vs, scale, ref = ref_of(case, "fp16")
    for a, b in zip(ref, VW.reference_and_bound(q, ks, vs, scale, "fp16")):
        assert np.array_equal(a, b)
    # zero-padding to D = 128 leaves the witness where it is (what the launch adds past D are exact zeros)
    pad = lambda x: np.concatenate([x, np.zeros(x.shape[:-1] + (128 - 72,), x.dtype)], axis=-1)        # noqa: E731
    po, pl = VW.witness(pad(q), [pad(k) for k in ks], [pad(v) for v in vs], scale)
    assert np.array_equal(pl, ref[1]) and np.array_equal(po[..., :72], ref[0]) and not po[..., 72:].any()


@pytest.mark.parametrize("dtype", list(TDT))
@pytest.mark.parametrize("plant", HC.PLANTS)
def test_planted_errors_exceed_the_bound_tenfold(plant, dtype):
    """every case that can show the error (HC.can_show: decided from the case alone) does, by 10 x the bound on at least one element of
    out or lse - so the GPU test's pass on these cases is not vacuous; where D makes the error impossible the plant returns the witness"""
    shown = {}
    for c in HC.CASES:
        q, ks, vs, scale, ref = ref_of(c, dtype)
        if not HC.can_show(plant, c):
            if c["D"] % 32 == 0:                                     # D = 96: whole k-steps, whole blocks, no padded width
                got = HC.planted(plant, q, ks, vs, scale)
                assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (plant, c["id"])
            continue
        fo, fl = VW.excess(*HC.planted(plant, q, ks, vs, scale), ref)
        assert max(fo, fl) >= 10.0, f"{plant} on {c['id']} {dtype}: only {fo:.2f} / {fl:.2f} x the bound (out / lse)"
        shown[c["D"]] = shown.get(c["D"], 0) + 1
    print(plant, dtype, shown)
    dims = [D for D in HC.DIMS if D % (32 if plant == "dropblock" else 16)]
    assert sorted(shown) == dims and all(n == len(HC.LENGTHS) for n in shown.values()), shown


@pytest.mark.parametrize("dtype", list(TDT))
def test_cpu_tensors_never_reach_a_launch(dtype, monkeypatch):
    """CPU tensors of head dim 72 .. 120: the eager definition, within the bound"""
    from compactfusion_amd.compact import attention as A
    monkeypatch.setattr(A, "_attn_fwd_native", lambda *a, **k: pytest.fail("CPU tensors reached the native launch"))
    monkeypatch.setattr(A, "_attn_fwd_native_var", lambda *a, **k: pytest.fail("CPU tensors reached the native launch"))
    assert A.ATTN_HEAD_DIMS == (64,) + HC.DIMS + (128,)
    for case in [c for c in HC.CASES if c["kind"] == "gauss"][::4]:
        q, ks, vs, scale, ref = ref_of(case, dtype)
        t = lambda x: torch.from_numpy(x).to(TDT[dtype])       # noqa: E731
        tq, tks, tvs = t(q), [t(k) for k in ks], [t(v) for v in vs]
        assert not A.attn_native_ok(tq, tks, tvs) and not A.attn_native_var_ok(tq, tks, tvs)
        out, lse = A.attention_blocks(tq, tks, tvs, scale)
        VW.check(out.float().numpy(), lse.transpose(1, 2).numpy(), ref, "attention_blocks, eager fallback")


def test_c_abi_argument_checks_without_a_gpu():
    """header, export and binding agree; every argument error in cfx_attn_fwd_blocks_var's order - NULL (sks and table entries included),
    flag bits, n / sizes / key counts / head dim / scale, alignment - returns before any launch: the count stays 0.  D = 64 and 128 are
    the other entry points', 76 and 136 nobody's: CFX_ERR_SHAPE"""
    from compactfusion_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(REPO, "include", "cfx.h")).read()
    assert re.search(r"\bint cfx_attn_fwd_blocks_hd\(cfx_ctx\* ctx, int n, const void\* q, const void\* const\* ks, const void\* const\* vs, const int\* sks,\s+"
                     r"int B, int Sq, int H, int D, float softmax_scale, unsigned flags, void\* out, void\* lse, void\* stream\);", hdr)
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT cfx_attn_fwd_blocks_hd\b", exported)
    bound = {n: a for n, _, a in _lib.SYMBOLS}
    assert bound["cfx_attn_fwd_blocks_hd"] == bound["cfx_attn_fwd_blocks_var"] and len(bound["cfx_attn_fwd_blocks_hd"]) == 15
    ctx = lib.cfx_create(0)
    assert ctx
    f = lib.cfx_attn_fwd_blocks_hd
    P, I = ctypes.c_void_p * 17, ctypes.c_int * 17
    ks = P(*[0x10000 + 0x1000 * i for i in range(17)])
    vs = P(*[0x40000 + 0x1000 * i for i in range(17)])
    sk = I(*[4 + i for i in range(17)])
    q, out, lse = 0x70000, 0x80000, 0x90000
    NULL, SHAPE, ALIGN, CODEC = -1, -2, -3, -4
    BF = _lib.ELEM_BF16

    def count():
        n = ctypes.c_ulonglong(99)
        assert lib.cfx_attn_fwd_launches(ctx, ctypes.byref(n)) == 0
        return n.value
    assert count() == 0
    # 1. NULL pointers, sks and table entries included - before anything else
    assert f(None, 2, q, ks, vs, sk, 1, 4, 2, 72, 0.125, 0, out, lse, None) == NULL
    assert f(ctx, 2, None, ks, vs, sk, 1, 4, 2, 72, 0.125, 0, out, lse, None) == NULL
    assert f(ctx, 2, q, None, vs, sk, 1, 4, 2, 72, 0.125, 0, out, lse, None) == NULL
    assert f(ctx, 2, q, ks, None, sk, 1, 4, 2, 72, 0.125, 0, out, lse, None) == NULL
    assert f(ctx, 2, q, ks, vs, None, 1, 4, 2, 72, 0.125, 0, out, lse, None) == NULL
    assert f(ctx, 2, q, ks, vs, None, 1, 4, 2, 64, -1.0, 0x40, 0x80002, lse, None) == NULL          # ... whatever else is wrong
    assert f(ctx, 2, q, ks, vs, sk, 1, 4, 2, 72, 0.125, 0, None, lse, None) == NULL
    assert f(ctx, 2, q, ks, vs, sk, 1, 4, 2, 72, 0.125, 0, out, None, None) == NULL
    assert b"null" in lib.cfx_last_error_string(ctx)
    for k in (0, 1, 15):
        holed = P(*[None if i == k else 0x10000 + 0x1000 * i for i in range(17)])
        assert f(ctx, 16, q, holed, vs, sk, 1, 4, 2, 72, 0.125, 0, out, lse, None) == NULL
        assert f(ctx, 16, q, ks, holed, sk, 1, 4, 2, 72, 0.125, 0, out, lse, None) == NULL
        assert f(ctx, 16, q, holed, vs, sk, 1, 4, 2, 64, -1.0, 0x40, 0x80002, lse, None) == NULL
    holed = P(*[None if i == 3 else 0x10000 + 0x1000 * i for i in range(17)])
    assert f(ctx, 3, q, holed, vs, sk, 1, 4, 2, 72, 0.125, 0x40, out, lse, None) == CODEC             # (entry 3 is not one of 3 blocks)
    # 2. flag bits: CFX_ELEM_BF16 only
    zero1 = I(*[0 if i == 1 else 4 for i in range(17)])
    for bad in (1, 2, 4, 0x40, 0x200, BF | 1, 0xFFFFFFFF):
        assert f(ctx, 2, q, ks, vs, sk, 1, 4, 2, 72, 0.125, bad, out, lse, None) == CODEC, bad
        assert f(ctx, 0, q, ks, vs, zero1, 1, 4, 2, 64, 0.0, bad, 0x80002, lse, None) == CODEC        # ... before n, the sizes, the scale, the alignment
    assert b"flag" in lib.cfx_last_error_string(ctx)
    # 3. n outside 1 .. 16, the sizes, a block without keys, the head dim, the launch's size, the scale - before the alignment
    for fl in (0, BF):
        for n in (0, 17, -1, 1 << 20):
            assert f(ctx, n, q, ks, vs, sk, 1, 4, 2, 72, 0.125, fl, 0x80002, lse, None) == SHAPE, (fl, n)
        for B, Sq, H, D in ((0, 4, 2, 72), (1, 0, 2, 72), (1, 4, 0, 72), (-1, 4, 2, 72), (1, 4, 2, 0), (1, 4, 2, 64), (1, 4, 2, 128), (1, 4, 2, 76),
                            (1, 4, 2, 136), (1, 4, 2, 32), (1, 4, 2, 100), (1, 4, 2, -72), (1, 4, 2, 256), (1 << 20, 1 << 20, 1 << 10, 72)):
            assert f(ctx, 2, q, ks, vs, sk, B, Sq, H, D, 0.125, fl, 0x80002, lse, None) == SHAPE, (B, Sq, H, D)
        for D in (64, 128, 76, 136):                                 # ... with everything else in order too
            assert f(ctx, 2, q, ks, vs, sk, 1, 4, 2, D, 0.125, fl, out, lse, None) == SHAPE, D
        assert b"head dim" in lib.cfx_last_error_string(ctx)
        for k in (0, 1, 15):
            for bad in (0, -1, -(1 << 31)):
                assert f(ctx, 16, q, ks, vs, I(*[bad if i == k else 4 for i in range(17)]), 1, 4, 2, 72, 0.125, fl, 0x80002, lse, None) == SHAPE, (k, bad)
        for sc in (0.0, -0.125, float("inf"), float("-inf"), float("nan")):
            assert f(ctx, 2, q, ks, vs, sk, 1, 4, 2, 72, sc, fl, 0x80002, lse, None) == SHAPE, sc
    # 4. 16-byte alignment of q, out, lse and of every block - every accepted D gets this far
    for D in HC.DIMS:
        assert f(ctx, 2, q, ks, vs, sk, 1, 4, 2, D, 0.125, 0, out + 8, lse, None) == ALIGN, D
    for bq, bo, bl in ((q + 2, out, lse), (q, out + 8, lse), (q, out, lse + 4)):
        assert f(ctx, 2, bq, ks, vs, sk, 1, 4, 2, 72, 0.125, 0, bo, bl, None) == ALIGN
    for k in (0, 7, 15):
        off = P(*[0x10000 + 0x1000 * i + (2 if i == k else 0) for i in range(17)])
        assert f(ctx, 16, q, off, vs, sk, 1, 4, 2, 72, 0.125, BF, out, lse, None) == ALIGN
        assert f(ctx, 16, q, ks, off, sk, 1, 4, 2, 72, 0.125, 0, out, lse, None) == ALIGN
    assert count() == 0
    lib.cfx_destroy(ctx)


def test_resource_rows_of_the_new_source():
    """cfx_attn_hd.hip alone: the 42 k_attn_fwd_blocks_hd instantiations (2 element types x 7 head dims x 3 query tiles) plus the
    k_copy_probe cfx_device.h puts in every translation unit; no scratch; VGPRs + AGPRs at most 512; LDS the D = 128 image - two K and two
    V tiles of 16 KiB, 64 KiB.  The source sits in a list of its own, built into and a dependency of both libraries; the other attention
    sources' lists are what they were."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import resource_usage as RU
    finally:
        sys.path.pop(0)
    from compactfusion_amd import build as B
    assert [os.path.basename(p) for p in B.ATTN_HD_SRC] == ["cfx_attn_hd.hip"]
    assert [os.path.basename(p) for p in B.ATTN_VAR_SRC] == ["cfx_attn_var.hip"] and [os.path.basename(p) for p in B.ATTN_SRC] == ["cfx_attn.hip"]
    assert not set(B.ATTN_HD_SRC) & (set(B.SRC) | set(B.CAPTURE_SRC) | set(B.MERGE_SRC) | set(B.ATTN_SRC) | set(B.ATTN_VAR_SRC))
    rows = RU._one(B.ATTN_HD_SRC[0])
    names = [re.sub(r"^void ", "", re.sub(r"\(.*$", "", d)) for d in RU.demangle([r["name"] for r in rows])]
    want = [f"k_attn_fwd_blocks_hd<{e}, {d}, {nw}>" for e in ("ElemF16", "ElemBF16") for d in HC.DIMS for nw in (2, 4, 8)]
    assert len(want) == 42 and sorted(names) == sorted(["k_copy_probe"] + want), names
    found = {}
    for r, name in zip(rows, names):
        assert r.get("scratch", 0) == 0, (name, r)
        assert r.get("vgpr", 0) + r.get("agpr", 0) <= 512, (name, r)
        if name != "k_copy_probe":
            assert r.get("lds", 0) == 4 * 64 * 256 == 65536, (name, r)
            found[name] = {k: r.get(k, 0) for k in ("vgpr", "agpr", "sgpr", "scratch", "lds", "occupancy")}
    recorded = json.load(open(os.path.join(REPO, "profiles", "attn_hd_rows.json")))["resource_rows"]
    assert recorded == found, "profiles/attn_hd_rows.json: resource_rows differ from what the compiler reports (tools/attn_hd_rows.py --resources rewrites them)"
    assert "ATTN_HD_SRC" in inspect.getsource(B.needs_build) and "ATTN_HD_SRC" in inspect.getsource(B.build_lib)
    src = open(B.ATTN_HD_SRC[0]).read()
    assert "asm" not in re.sub(r"//.*", "", src)                     # plain HIP and builtins


# ---- patch_gather_fwd on CPU stand-ins: which calls a layer makes ------------------------------------------------------------------------
WP, PSHAPE, PJ = 2, (1, 6, 2, 72), (1, 3, 2, 72)


class _TorchSpy:
    """stands in for compact/patchpara/fwd.py's `torch`: counts torch.cat, passes everything through"""

    def __init__(self):
        self.cats = 0

    def cat(self, *a, **kw):
        self.cats += 1
        return torch.cat(*a, **kw)

    def __getattr__(self, name):
        return getattr(torch, name)


@pytest.fixture
def patch_layer(monkeypatch):
    """patch_gather_fwd of a logical world looped back on CPU tensors (the raw synchronous and the async gather), stand-ins for the two
    launches (the eager definition) and for the two `attn_native*_ok` (the conditions on shapes only), spies on block_attention and
    torch.cat"""
    from compactfusion_amd import config
    from compactfusion_amd.compact import attention as A
    from compactfusion_amd.compact import main as cm
    from compactfusion_amd.compact.patchpara import fwd as F
    from compactfusion_amd.compact import CompactConfig, PatchConfig
    calls = []
    state = {"world": WP, "ok": True}
    spy = _TorchSpy()

    class Done:
        def wait(self):
            pass

    def gather(recv, send, group=None, async_op=False):
        recv.view(state["world"], -1).copy_(send.view(1, -1).expand(state["world"], -1))
        return Done()

    def launch(name):
        def f(q_, ks, vs, scale, tabs=None):
            calls.append((name, list(ks), list(vs), scale))
            return eager(q_, ks, vs, scale)                          # CPU tensors: the eager definition
        return f
    eager = A.attention_blocks

    def same(q_, ks, vs):
        return state["ok"] and all(t.shape == ks[0].shape for t in list(ks) + list(vs))

    def spied_attention(*a, **kw):
        calls.append(("block_attention", a[1], a[2], a[4]))
        return A.block_attention(*a, **kw)
    monkeypatch.setattr(F, "torch", spy)
    monkeypatch.setattr(F.dist, "get_world_size", lambda g=None: state["world"])
    monkeypatch.setattr(F.dist, "get_rank", lambda g=None: 0)
    monkeypatch.setattr(F.dist, "all_gather_into_tensor", gather)
    monkeypatch.setattr(F, "attn_native_ok", same)
    monkeypatch.setattr(F, "attn_native_var_ok", lambda q_, ks, vs: state["ok"] and all(k.shape == v.shape for k, v in zip(ks, vs)))
    monkeypatch.setattr(F, "_attn_fwd_native", launch("launch"))
    monkeypatch.setattr(F, "_attn_fwd_native_var", launch("launch_var"))
    monkeypatch.setattr(F, "block_attention", spied_attention)
    monkeypatch.setattr(A, "attention_blocks", (lambda real: lambda *a, **k: (calls.append(("attention_blocks",)), real(*a, **k))[1])(A.attention_blocks))
    F._buffers.clear()

    def init(async_comm):
        cm.compact_init(CompactConfig(enabled=True, override_with_patch_gather_fwd=True, patch_gather_fwd_config=PatchConfig(False, async_comm, 1),
                                      compress_func=lambda l, s: None, comp_rank=-1))
    g = torch.Generator().manual_seed(3)
    rnd = lambda shape: torch.randn(shape, generator=g).to(torch.float16)       # noqa: E731
    config.reset()
    yield F, init, rnd, calls, state, spy
    config.reset()
    F._buffers.clear()


def _whole(q, ks, vs, scale):
    from compactfusion_amd.compact import attention as A
    return A.block_attention(q, torch.cat(ks, dim=1), torch.cat(vs, dim=1), 0.0, scale, causal=False)


@pytest.mark.parametrize("async_comm", [False, True])
@pytest.mark.parametrize("joint", ["none", "front", "rear"])
def test_patch_gather_fwd_goes_native_only_when_the_launch_takes_the_call(patch_layer, joint, async_comm):
    """configure(attention="native"): ONE launch over [joint] + states (front), states + [joint] (rear) or the states alone - the
    equal-length entry without joint tensors, the unequal-length one with them -, the gathered states themselves (no copy), no torch.cat
    anywhere in fwd.py, in the synchronous and the async (warm-up and steady) raw gather.  The default setting, a causal call, dropout, a
    window, 17 blocks and a call the launch does not take keep cat + SDPA - and never reach `attention_blocks`' eager definition."""
    import compactfusion_amd
    F, init, rnd, calls, state, spy = patch_layer
    q, k, v, jk, jv = rnd(PSHAPE), rnd(PSHAPE), rnd(PSHAPE), rnd(PJ), rnd(PJ)
    scale = PSHAPE[-1] ** -0.5
    kw = dict(joint_tensor_key=jk, joint_tensor_value=jv, joint_strategy=joint) if joint != "none" else {}
    nb = WP + (joint != "none")
    launch = "launch" if joint == "none" else "launch_var"

    def run(step=0, **over):
        del calls[:]
        spy.cats = 0
        args = dict(causal=False, mod_idx=4, current_iter=step, **kw)
        args.update(over)
        return F.patch_gather_fwd(q, k, v, **args)
    # the default setting: today's lines
    init(async_comm)
    want = run(0)
    assert [c[0] for c in calls] == ["block_attention"] and spy.cats >= 3 and tuple(calls[0][1].shape)[1] == WP * PSHAPE[1] + (PJ[1] if kw else 0)
    compactfusion_amd.configure(attention="native")
    init(async_comm)
    for step in (0, 1, 2):                                           # (async: step 0 gathers synchronously, steps 1, 2 consume the previous gather)
        got = run(step)
        assert [c[0] for c in calls] == [launch], (step, [c[0] for c in calls])
        assert spy.cats == 0, f"step {step}: torch.cat called {spy.cats} times from fwd.py"
        _, lk, lv, lscale = calls[0]
        assert len(lk) == len(lv) == nb and lscale == scale
        states_k = lk[1:] if joint == "front" else (lk[:-1] if joint == "rear" else lk)
        states_v = lv[1:] if joint == "front" else (lv[:-1] if joint == "rear" else lv)
        if joint == "front":
            assert lk[0] is jk and lv[0] is jv
        if joint == "rear":
            assert lk[-1] is jk and lv[-1] is jv
        assert all(torch.equal(t, k) for t in states_k) and all(torch.equal(t, v) for t in states_v)           # looped back: every rank's shard is ours
        assert got[2] is None and got[0].dtype == q.dtype and tuple(got[0].shape) == PSHAPE and tuple(got[1].shape) == (PSHAPE[0], PSHAPE[2], PSHAPE[1])
        assert torch.allclose(got[0].float(), want[0].float(), atol=2e-3, rtol=2e-3) and torch.allclose(got[1], want[1], atol=1e-4, rtol=1e-5)
    # what the launch cannot take keeps cat + SDPA
    init(False)
    for over in (dict(causal=True), dict(dropout_p=0.1), dict(window_size=(3, 3)), dict(window_size=(-1, 0))):
        run(0, **over)
        assert [c[0] for c in calls] == ["block_attention"] and spy.cats >= 2, over
    state["ok"] = False
    run(0)
    assert [c[0] for c in calls] == ["block_attention"] and spy.cats >= 2
    state["ok"] = True
    run(0)
    assert [c[0] for c in calls] == [launch]
    state["world"] = 16 if kw else 17                                # 17 blocks with the joint one
    F._buffers.clear()
    run(0)
    assert [c[0] for c in calls] == ["block_attention"] and tuple(calls[0][1].shape)[1] == state["world"] * PSHAPE[1] + (PJ[1] if kw else 0)
    state["world"] = 15 if kw else 16                                # 16 fit
    F._buffers.clear()
    run(0)
    assert [c[0] for c in calls] == [launch] and len(calls[0][1]) == 16
