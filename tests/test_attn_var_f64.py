"""The native attention forward over K,V blocks of UNEQUAL length (cfx_attn_fwd_blocks_var, attention_blocks, configure(joint=...)) on the
CPU: the witness and bound of tests/_attn_var_f64.py against tests/_attn_f64.py's on equal lengths; the case list's own conditions; the
eager fallback on every case; planted errors, each at least 10 x the bound on every case that can show it; the C-ABI's argument checks;
the `joint` setting; the calls `_blocks*` make with joint tensors; the new source's resource rows.  No GPU."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import _attn_cases as C
import _attn_f64 as W
import _attn_var_cases as VC
import _attn_var_f64 as VW

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c["id"] for c in VC.CASES]
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
_refs = {}


def ref_of(case, dtype):
    """the case's inputs and its witness / bound, computed once"""
    key = (case["id"], dtype)
    if key not in _refs:
        q, ks, vs, scale = VC.build(case, dtype)
        _refs[key] = (q, ks, vs, scale, VW.reference_and_bound(q, ks, vs, scale, dtype))
    return _refs[key]


def test_witness_and_bound_equal_the_equal_length_ones():
    """on blocks of one length T = n ceil(Sk / 64): the same reference and the same bound, number for number"""
    assert VW.witness is W.witness and VW.check is W.check and VW.excess is W.excess and VW.scores is W.scores
    assert (VW.U, VW.SLACK, VW.EPS, VW.SUB) == (W.U, W.SLACK, W.EPS, W.SUB)
    for case in [c for c in C.CASES if c["kind"] in ("gauss", "peak", "ramp")][::3]:
        for dtype in TDT:
            q, ks, vs, scale = C.build(case, dtype)
            assert VW.tiles(k.shape[1] for k in ks) == case["n"] * ((case["Sk"] + 63) // 64)
            for a, b in zip(VW.reference_and_bound(q, ks, vs, scale, dtype), W.reference_and_bound(q, ks, vs, scale, dtype)):
                assert np.array_equal(a, b), case["id"]
    assert VW.tiles([65, 64, 63]) == 4 and VW.tiles([100, 37, 128, 5]) == 6 and VW.tiles(range(1, 17)) == 16 and VW.tiles([64, 128, 192]) == 6


def test_case_list_covers_what_it_claims():
    cs = VC.CASES
    assert len(set(IDS)) == len(cs) and 40 <= len(cs) <= 70
    assert all(c["H"] == 2 for c in cs) and {c["Sq"] for c in cs} == {1, 33, 80, 129} and {c["kind"] for c in cs} == {"gauss", "peak", "ramp"}
    want = [[1], [64, 1], [1, 64], [65, 64, 63], [16, 64, 64, 64], [64, 64, 64, 16], [130, 40, 40], [100, 37, 128, 5], list(range(1, 17)), [64, 128, 192]]
    gauss64 = [c for c in cs if c["kind"] == "gauss" and c["D"] == 64]
    assert [c["sks"] for c in gauss64] == want                                       # every length list, gaussian, D = 64
    assert sum(c["B"] == 2 for c in gauss64) * 2 >= len(gauss64) and sum(c["B"] == 2 for c in cs) * 2 >= len(cs)       # B = 2 on at least half
    d128 = [c for c in cs if c["D"] == 128]
    assert 3 <= len(d128) <= 8 and {c["kind"] for c in d128} == {"gauss", "peak", "ramp"}                               # D = 128 on a handful only
    for sks in VC.PEAK_LISTS:                                                         # the designated key at the first and last key of every block
        got = {VC.peak_position(c) for c in cs if c["kind"] == "peak" and c["sks"] == sks and c["D"] == 64}
        assert got == {(b, k) for b, n in enumerate(sks) for k in (0, n - 1)}, (sks, got)
    assert any(c["B"] == 2 and len(set(c["sks"])) > 1 for c in cs if c["kind"] == "peak")
    for dtype in TDT:
        for c in cs:
            q, ks, vs, scale, (ro, rl, ob, lb) = ref_of(c, dtype)
            assert [k.shape for k in ks] == [(c["B"], n, 2, c["D"]) for n in c["sks"]] == [v.shape for v in vs] and q.shape == (c["B"], c["Sq"], 2, c["D"])
            if c["kind"] == "peak":                                  # the designated key carries more than 0.9 of every row
                s, _ = W.scores(q, ks, scale)
                blk, key = VC.peak_position(c)
                w = np.exp(s - rl.transpose(0, 2, 1)[..., None])
                assert w[..., sum(c["sks"][:blk]) + key].min() > 0.9, c["id"]
            if c["kind"] == "ramp":                                  # block maxima rise and fall by up to 1e4
                s, _ = W.scores(q, ks, scale)
                assert s.max() > 9000 and (s.min() < -9000 or len(c["sks"]) < 4), c["id"]


@pytest.mark.parametrize("dtype", list(TDT))
@pytest.mark.parametrize("case", VC.CASES, ids=IDS)
def test_eager_fallback_meets_the_bound(case, dtype, monkeypatch):
    """CPU tensors of unequal length: the eager definition, never a launch"""
    from compactfusion_amd.compact import attention as A
    monkeypatch.setattr(A, "_attn_fwd_native", lambda *a, **k: pytest.fail("CPU tensors reached the native launch"))
    monkeypatch.setattr(A, "_attn_fwd_native_var", lambda *a, **k: pytest.fail("CPU tensors reached the native launch"))
    q, ks, vs, scale, ref = ref_of(case, dtype)
    t = lambda x: torch.from_numpy(x).to(TDT[dtype])       # noqa: E731
    tq, tks, tvs = t(q), [t(k) for k in ks], [t(v) for v in vs]
    assert not A.attn_native_var_ok(tq, tks, tvs)
    out, lse = A.attention_blocks(tq, tks, tvs, scale)
    B, Sq, H, D = q.shape
    assert out.dtype == TDT[dtype] and tuple(out.shape) == (B, Sq, H, D) and tuple(lse.shape) == (B, H, Sq)
    fo, fl = VW.check(out.float().numpy(), lse.transpose(1, 2).numpy(), ref, "attention_blocks, eager fallback")
    print(f"{case['id']} {dtype}: eager fallback {fo:.3f} / {fl:.3f} of the bound (out / lse)")


@pytest.mark.parametrize("dtype", list(TDT))
@pytest.mark.parametrize("plant", VW.PLANTS)
def test_planted_errors_exceed_the_bound_tenfold(plant, dtype):
    """every case whose lengths and values can show the error (VW.can_show: decided from the case alone) does, by 10 x the bound on at
    least one element of out or lse - so the GPU test's pass on these cases is not vacuous; every kind that can show it at all does"""
    shown = {}
    for c in VC.CASES:
        if not VW.can_show(plant, c):
            continue
        q, ks, vs, scale, ref = ref_of(c, dtype)
        fo, fl = VW.excess(*VW.planted(plant, q, ks, vs, scale), ref)
        assert max(fo, fl) >= 10.0, f"{plant} on {c['id']} {dtype}: only {fo:.2f} / {fl:.2f} x the bound (out / lse)"
        shown[c["kind"]] = shown.get(c["kind"], 0) + 1
    print(plant, dtype, shown)
    assert shown.get("gauss", 0) >= 5 and shown.get("peak", 0) >= 2, f"{plant}: only {shown} cases can show it"
    if plant == "stride0":                                 # the batch stride shows only at b = 1
        assert all(c["B"] == 2 for c in VC.CASES if VW.can_show(plant, c))


def test_planted_errors_leave_equal_blocks_alone():
    """the four index errors are errors of UNEQUAL lengths: on equal blocks they return the witness itself (droplast aside)"""
    case = dict(B=2, Sq=33, sks=[40, 40, 40], H=2, D=64, kind="gauss", id="equal-gauss")
    q, ks, vs, scale = VC.build(case, "fp16")
    want = VW.witness(q, ks, vs, scale)
    for plant in ("mask_next", "mask_prev", "stride0"):
        assert not VW.can_show(plant, case)
        got = VW.planted(plant, q, ks, vs, scale)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), plant
    assert not VW.can_show("jointend", case)               # (a permutation of equal blocks: the same keys in another order)
    got = VW.planted("jointend", q, ks, vs, scale)
    assert np.allclose(got[0], want[0], rtol=1e-12, atol=1e-12) and np.allclose(got[1], want[1], rtol=1e-12)


def test_c_abi_argument_checks_without_a_gpu():
    """header, export and binding agree; every argument error in the documented order - NULL (sks and table entries included), flag bits,
    n / sizes / key counts / scale, alignment (a pending gate error needs a device) - returns before any launch: the count stays 0"""
    from compactfusion_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(REPO, "include", "cfx.h")).read()
    assert re.search(r"\bint cfx_attn_fwd_blocks_var\(cfx_ctx\* ctx, int n, const void\* q, const void\* const\* ks, const void\* const\* vs, const int\* sks,\s+"
                     r"int B, int Sq, int H, int D, float softmax_scale, unsigned flags, void\* out, void\* lse, void\* stream\);", hdr)
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT cfx_attn_fwd_blocks_var\b", exported)
    bound = {n: a for n, _, a in _lib.SYMBOLS}
    assert len(bound["cfx_attn_fwd_blocks_var"]) == 15 and lib.cfx_abi_version() == 2
    ctx = lib.cfx_create(0)
    assert ctx
    f = lib.cfx_attn_fwd_blocks_var
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
    assert f(None, 2, q, ks, vs, sk, 1, 4, 2, 64, 0.125, 0, out, lse, None) == NULL
    assert f(ctx, 2, None, ks, vs, sk, 1, 4, 2, 64, 0.125, 0, out, lse, None) == NULL
    assert f(ctx, 2, q, None, vs, sk, 1, 4, 2, 64, 0.125, 0, out, lse, None) == NULL
    assert f(ctx, 2, q, ks, None, sk, 1, 4, 2, 64, 0.125, 0, out, lse, None) == NULL
    assert f(ctx, 2, q, ks, vs, None, 1, 4, 2, 64, 0.125, 0, out, lse, None) == NULL
    assert f(ctx, 2, q, ks, vs, None, 1, 4, 2, 20, -1.0, 0x40, 0x80002, lse, None) == NULL          # ... whatever else is wrong
    assert f(ctx, 2, q, ks, vs, sk, 1, 4, 2, 64, 0.125, 0, None, lse, None) == NULL
    assert f(ctx, 2, q, ks, vs, sk, 1, 4, 2, 64, 0.125, 0, out, None, None) == NULL
    assert b"null" in lib.cfx_last_error_string(ctx)
    for k in (0, 1, 15):
        holed = P(*[None if i == k else 0x10000 + 0x1000 * i for i in range(17)])
        assert f(ctx, 16, q, holed, vs, sk, 1, 4, 2, 64, 0.125, 0, out, lse, None) == NULL
        assert f(ctx, 16, q, ks, holed, sk, 1, 4, 2, 64, 0.125, 0, out, lse, None) == NULL
        assert f(ctx, 16, q, holed, vs, sk, 1, 4, 2, 20, -1.0, 0x40, 0x80002, lse, None) == NULL
    holed = P(*[None if i == 3 else 0x10000 + 0x1000 * i for i in range(17)])
    assert f(ctx, 3, q, holed, vs, sk, 1, 4, 2, 64, 0.125, 0x40, out, lse, None) == CODEC             # (entry 3 is not one of 3 blocks)
    # 2. flag bits: CFX_ELEM_BF16 only
    zero1 = I(*[0 if i == 1 else 4 for i in range(17)])
    for bad in (1, 2, 4, 0x40, 0x200, BF | 1, 0xFFFFFFFF):
        assert f(ctx, 2, q, ks, vs, sk, 1, 4, 2, 64, 0.125, bad, out, lse, None) == CODEC, bad
        assert f(ctx, 0, q, ks, vs, zero1, 1, 4, 2, 20, 0.0, bad, 0x80002, lse, None) == CODEC        # ... before n, the sizes, the scale, the alignment
    assert b"flag" in lib.cfx_last_error_string(ctx)
    # 3. n outside 1 .. 16, the sizes, a block without keys, the head dim, the launch's size, the scale - before the alignment
    for fl in (0, BF):
        for n in (0, 17, -1, 1 << 20):
            assert f(ctx, n, q, ks, vs, sk, 1, 4, 2, 64, 0.125, fl, 0x80002, lse, None) == SHAPE, (fl, n)
        for B, Sq, H, D in ((0, 4, 2, 64), (1, 0, 2, 64), (1, 4, 0, 64), (-1, 4, 2, 64), (1, 4, 2, 0), (1, 4, 2, 32), (1, 4, 2, 96), (1, 4, 2, 256),
                            (1, 4, 2, -64), (1 << 20, 1 << 20, 1 << 10, 64)):
            assert f(ctx, 2, q, ks, vs, sk, B, Sq, H, D, 0.125, fl, 0x80002, lse, None) == SHAPE, (B, Sq, H, D)
        for k in (0, 1, 15):
            for bad in (0, -1, -(1 << 31)):
                assert f(ctx, 16, q, ks, vs, I(*[bad if i == k else 4 for i in range(17)]), 1, 4, 2, 64, 0.125, fl, 0x80002, lse, None) == SHAPE, (k, bad)
        for sc in (0.0, -0.125, float("inf"), float("-inf"), float("nan")):
            assert f(ctx, 2, q, ks, vs, sk, 1, 4, 2, 64, sc, fl, 0x80002, lse, None) == SHAPE, sc
    # 4. 16-byte alignment of q, out, lse and of every block
    for bq, bo, bl in ((q + 2, out, lse), (q, out + 8, lse), (q, out, lse + 4)):
        assert f(ctx, 2, bq, ks, vs, sk, 1, 4, 2, 64, 0.125, 0, bo, bl, None) == ALIGN
    for k in (0, 7, 15):
        off = P(*[0x10000 + 0x1000 * i + (2 if i == k else 0) for i in range(17)])
        assert f(ctx, 16, q, off, vs, sk, 1, 4, 2, 64, 0.125, BF, out, lse, None) == ALIGN
        assert f(ctx, 16, q, ks, off, sk, 1, 4, 2, 64, 0.125, 0, out, lse, None) == ALIGN
    assert count() == 0
    lib.cfx_destroy(ctx)


def test_resource_rows_of_the_new_source():
    """cfx_attn_var.hip alone: the twelve k_attn_fwd_blocks_var instantiations (2 element types x 2 head dims x 3 query tiles) plus the
    k_copy_probe cfx_device.h puts in every translation unit; no scratch; VGPRs + AGPRs at most 512; LDS the two K and two V tiles, at most
    64 KiB.  The source sits in a list of its own, built into and a dependency of both libraries; cfx_attn.hip's list is what it was."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import resource_usage as RU
    finally:
        sys.path.pop(0)
    from compactfusion_amd import build as B
    assert [os.path.basename(p) for p in B.ATTN_VAR_SRC] == ["cfx_attn_var.hip"] and [os.path.basename(p) for p in B.ATTN_SRC] == ["cfx_attn.hip"]
    assert not set(B.ATTN_VAR_SRC) & (set(B.SRC) | set(B.CAPTURE_SRC) | set(B.MERGE_SRC) | set(B.ATTN_SRC))
    rows = RU._one(B.ATTN_VAR_SRC[0])
    names = [re.sub(r"^void ", "", re.sub(r"\(.*$", "", d)) for d in RU.demangle([r["name"] for r in rows])]
    want = [f"k_attn_fwd_blocks_var<{e}, {d}, {nw}>" for e in ("ElemF16", "ElemBF16") for d in (64, 128) for nw in (2, 4, 8)]
    assert sorted(names) == sorted(["k_copy_probe"] + want), names
    found = {}
    for r, name in zip(rows, names):
        assert r.get("scratch", 0) == 0, (name, r)
        assert r.get("vgpr", 0) + r.get("agpr", 0) <= 512, (name, r)
        if name != "k_copy_probe":
            d = int(name.split(",")[1])
            assert r.get("lds", 0) == 4 * 64 * d * 2 <= 65536, (name, r)
            found[name] = {k: r.get(k, 0) for k in ("vgpr", "agpr", "sgpr", "scratch", "lds", "occupancy")}
    recorded = json.load(open(os.path.join(REPO, "profiles", "attn_joint_rows.json")))["resource_rows"]
    assert recorded == found, "profiles/attn_joint_rows.json: resource_rows differ from what the compiler reports (tools/attn_joint_rows.py --resources rewrites them)"
    import inspect
    assert "ATTN_VAR_SRC" in inspect.getsource(B.needs_build) and "ATTN_VAR_SRC" in inspect.getsource(B.build_lib)


def test_configure_joint(monkeypatch):
    import compactfusion_amd
    from compactfusion_amd import config
    config.reset()
    try:
        monkeypatch.delenv("CFX_JOINT", raising=False)
        assert config.get("joint") == "general" and compactfusion_amd.configure()["joint"] == "general"
        monkeypatch.setenv("CFX_JOINT", "steady")
        assert config.get("joint") == "steady"
        assert compactfusion_amd.configure(joint="general")["joint"] == "general"                # an explicit configure() overrides it
        assert compactfusion_amd.configure(joint="steady")["joint"] == "steady"
        with pytest.raises(ValueError):
            compactfusion_amd.configure(joint="front")
        assert config.get("joint") == "steady"
        config.reset()
        monkeypatch.setenv("CFX_JOINT", "native")
        with pytest.raises(ValueError):
            config.get("joint")
    finally:
        config.reset()
    assert "CFX_JOINT" in config.__doc__ and "cfx_attn_fwd_blocks_var" in config.__doc__
    assert "CFX_JOINT" in open(os.path.join(REPO, "INTEGRATION.md")).read()


# ---- _blocks on CPU stand-ins: which calls a joint call makes ---------------------------------------------------------------------------
WR, SHAPE, QSHAPE, JSHAPE = 4, (1, 6, 2, 16), (1, 9, 2, 16), (1, 3, 2, 16)


@pytest.fixture
def layer(monkeypatch):
    """a steady layer of WR ranks with CPU tensors for its peers' states; stand-ins for the two launches (the eager definition) and spies
    on everything compact/ring.py calls around them"""
    from compactfusion_amd import config
    from compactfusion_amd.compact import attention as A
    from compactfusion_amd.compact import ring as R
    g = torch.Generator().manual_seed(12)
    rnd = lambda shape: torch.randn(shape, generator=g).to(torch.float16)       # noqa: E731
    q, k, v, jk, jv = rnd(QSHAPE), rnd(SHAPE), rnd(SHAPE), rnd(JSHAPE), rnd(JSHAPE)
    peers = [(s, rnd(SHAPE), rnd(SHAPE)) for s in range(1, WR)]
    st = R._SteadyLayer.__new__(R._SteadyLayer)
    st.world, st._peers, st._fast = WR, peers, False
    calls = []
    backend = {"ok": True}

    def launch(name):
        def f(q_, ks, vs, scale, tabs=None):
            calls.append((name, (q_, list(ks), list(vs), scale, tabs)))
            return A.attention_blocks(q_, ks, vs, scale)             # CPU tensors: the eager definition
        return f

    def spied(name, fn):
        def wrap(*a, **kw):
            calls.append((name, a))
            return fn(*a, **kw)
        return wrap
    monkeypatch.setattr(R, "attn_native_ok", lambda q_, ks, vs: backend["ok"])
    monkeypatch.setattr(R, "_attn_fwd_native", launch("launch"))
    monkeypatch.setattr(R, "_attn_fwd_native_var", launch("launch_var"))
    monkeypatch.setattr(R, "merge_blocks", spied("merge_blocks", A.merge_blocks))
    monkeypatch.setattr(R, "update_out_and_lse", spied("update_out_and_lse", A.update_out_and_lse))
    monkeypatch.setattr(R, "block_attention", spied("block_attention", A.block_attention))
    monkeypatch.setattr(R, "flag_wait", lambda wait, device: calls.append(("flag_wait", wait)))
    monkeypatch.setattr(A, "flag_wait", lambda wait, device: calls.append(("flag_wait(in merge)", wait)))
    monkeypatch.setattr(R, "_with_joint", spied("with_joint", R._with_joint))
    config.reset()
    yield st, q, k, v, jk, jv, peers, calls, backend
    config.reset()


def _whole(q, ks, vs, scale):
    from compactfusion_amd.compact import attention as A
    return A.attention_blocks(q, [torch.cat(ks, dim=1)], [torch.cat(vs, dim=1)], scale)


@pytest.mark.parametrize("strategy", ["front", "rear"])
@pytest.mark.parametrize("merge", ["chain", "once"])
@pytest.mark.parametrize("lane", [False, True])
def test_blocks_sdpa_attends_joint_with_the_first_or_last_block(layer, lane, merge, strategy):
    """attention="sdpa": the calls of a call without joint tensors, one for one - W block_attention calls, the same merges, `issue` and
    waits - with block 0 = [joint ; own] (front) or block W-1 = [peer ; joint] (rear); the result is the attention over all keys"""
    import compactfusion_amd
    st, q, k, v, jk, jv, peers, calls, backend = layer
    flagf = lambda r: 0x1000 + 64 * r        # noqa: E731
    args = (lambda s, lean: calls.append(("issue", (s, lean))), flagf, 5) if lane else (None, None, 0)
    scale = q.shape[-1] ** -0.5
    compactfusion_amd.configure(attention="sdpa", attn_merge=merge)
    st._blocks(q, k, v, scale, None, *args)
    plain = [(c[0], c[1] if c[0] in ("issue", "flag_wait", "flag_wait(in merge)") else None) for c in calls]
    del calls[:]
    got = st._blocks(q, k, v, scale, None, *args, (jk, jv, strategy))
    names = [c[0] for c in calls]
    assert names.count("with_joint") == 1
    if lane and strategy == "rear":              # peer W-1's state is read - concatenated - only behind the wait for its flag
        waited = [i for i, c in enumerate(calls) if c[0].startswith("flag_wait") and c[1] == (flagf(WR - 1), 5)]
        assert len(waited) == 1 and waited[0] < names.index("with_joint") < [i for i, n in enumerate(names) if n == "block_attention"][-1]
    if strategy == "front":
        assert names.index("with_joint") < names.index("block_attention")
    calls[:] = [c for c in calls if c[0] != "with_joint"]
    assert [(c[0], c[1] if c[0] in ("issue", "flag_wait", "flag_wait(in merge)") else None) for c in calls] == plain
    assert not [c for c in calls if c[0].startswith("launch")]
    att = [c[1] for c in calls if c[0] == "block_attention"]
    assert len(att) == WR and all(a[0] is q for a in att)
    blocks_k, blocks_v = [k] + [p[1] for p in peers], [v] + [p[2] for p in peers]
    i = 0 if strategy == "front" else WR - 1
    blocks_k[i] = torch.cat([jk, blocks_k[i]], dim=1) if i == 0 else torch.cat([blocks_k[i], jk], dim=1)
    blocks_v[i] = torch.cat([jv, blocks_v[i]], dim=1) if i == 0 else torch.cat([blocks_v[i], jv], dim=1)
    for a, kk, vv in zip(att, blocks_k, blocks_v):
        assert torch.equal(a[1], kk) and torch.equal(a[2], vv)
    for j, a in enumerate(att):                                      # the untouched blocks are the tensors themselves, not copies
        if j != i:
            assert a[1] is blocks_k[j] and a[2] is blocks_v[j]
    want = _whole(q, blocks_k, blocks_v, scale)
    assert got[2] is None and got[0].dtype == q.dtype and tuple(got[0].shape) == QSHAPE and tuple(got[1].shape) == (QSHAPE[0], QSHAPE[2], QSHAPE[1])
    assert torch.allclose(got[0].float(), want[0].float(), atol=2e-3, rtol=2e-3) and torch.allclose(got[1], want[1], atol=1e-4, rtol=1e-5)


@pytest.mark.parametrize("strategy", ["front", "rear"])
@pytest.mark.parametrize("lane", [False, True])
def test_blocks_native_puts_joint_into_the_one_launch(layer, lane, strategy):
    """attention="native": the whole chain, a stand-alone wait per peer flag, then ONE cfx_attn_fwd_blocks_var launch over
    [joint, own, peers...] (front) or [own, peers..., joint] (rear) with per-block key counts; the peers' entries prepared once, the joint
    and own entries set by every call; the same layer serves calls without joint tensors in between"""
    import compactfusion_amd
    st, q, k, v, jk, jv, peers, calls, backend = layer
    flagf = lambda r: 0x1000 + 64 * r        # noqa: E731
    args = (lambda s, lean: calls.append(("issue", (s, lean))), flagf, 5) if lane else (None, None, 0)
    scale = q.shape[-1] ** -0.5
    compactfusion_amd.configure(attention="native")
    got = st._blocks(q, k, v, scale, None, *args, (jk, jv, strategy))
    names = [c[0] for c in calls]
    if lane:
        assert names == ["issue"] * WR + ["flag_wait"] * (WR - 1) + ["launch_var"], names
        assert [c[1] for c in calls[:WR]] == [(s, True) for s in range(WR)]
        assert [c[1] for c in calls[WR:2 * WR - 1]] == [(flagf(s), 5) for s in range(1, WR)]
    else:
        assert names == ["launch_var"], names
    lq, lks, lvs, lscale, tabs = calls[-1][1]
    rest_k, rest_v = [k] + [p[1] for p in peers], [v] + [p[2] for p in peers]
    want_k, want_v = ([jk] + rest_k, [jv] + rest_v) if strategy == "front" else (rest_k + [jk], rest_v + [jv])
    assert lq is q and lscale == scale and len(lks) == len(lvs) == WR + 1
    assert all(a is b for a, b in zip(lks, want_k)) and all(a is b for a, b in zip(lvs, want_v))
    assert len(tabs) == 3 and [p for p in tabs[0]] == [t.data_ptr() for t in want_k] and [p for p in tabs[1]] == [t.data_ptr() for t in want_v]
    assert [n for n in tabs[2]] == [t.shape[1] for t in want_k]
    want = _whole(q, want_k, want_v, scale)
    assert got[2] is None and torch.allclose(got[0].float(), want[0].float(), atol=2e-3, rtol=2e-3) and torch.allclose(got[1], want[1], atol=1e-4, rtol=1e-5)
    # a call without joint tensors in between: the equal-length launch on the layer's own tables
    del calls[:]
    st._blocks(q, k, v, scale, None, *args)
    assert [c[0] for c in calls if c[0].startswith("launch")] == ["launch"] and len(calls[-1][1][1]) == WR
    # another joint call, another length: the same table objects, the joint and own entries rewritten
    k2, v2, jk2, jv2 = k.clone(), v.clone(), torch.cat([jk, jk], dim=1), torch.cat([jv, jv], dim=1)
    del calls[:]
    st._blocks(q, k2, v2, scale, None, *args, (jk2, jv2, strategy))
    ji, oi = (0, 1) if strategy == "front" else (WR, 0)
    t2 = calls[-1][1][4]
    assert calls[-1][0] == "launch_var" and all(a is b for a, b in zip(t2, tabs))
    assert t2[0][ji] == jk2.data_ptr() and t2[1][ji] == jv2.data_ptr() and t2[2][ji] == 2 * JSHAPE[1] and t2[0][oi] == k2.data_ptr() and t2[1][oi] == v2.data_ptr()
    assert t2[0][oi + 1] == peers[0][1].data_ptr() and t2[2][oi + 1] == SHAPE[1]
    other = "rear" if strategy == "front" else "front"              # the other strategy on the same layer: tables of its own
    st._blocks(q, k, v, scale, None, *args, (jk, jv, other))
    assert calls[-1][0] == "launch_var" and calls[-1][1][4][0] is not tabs[0]


def test_blocks_native_with_joint_falls_back_to_the_sdpa_form(layer):
    """what the launch cannot take keeps the sdpa form: the stand-in saying no, and W + 1 > 16 blocks"""
    import compactfusion_amd
    st, q, k, v, jk, jv, peers, calls, backend = layer
    scale = q.shape[-1] ** -0.5
    compactfusion_amd.configure(attention="native")
    backend["ok"] = False
    st._blocks(q, k, v, scale, None, None, None, 0, (jk, jv, "front"))
    assert [c[0] for c in calls] == ["with_joint"] + ["block_attention", "update_out_and_lse"] * WR
    backend["ok"] = True
    st16 = type(st).__new__(type(st))
    st16.world, st16._peers, st16._fast = 16, (peers * 5), False
    assert st16._native_ok(q, k, v) is True and st16._native_joint_ok(q, k, v, (jk, jv, "rear")) is False      # 16 blocks fit, 17 do not
    del calls[:]
    st16._blocks(q, k, v, scale, None, None, None, 0, (jk, jv, "rear"))
    assert [c[0] for c in calls if c[0] != "with_joint"] == ["block_attention", "update_out_and_lse"] * 16


def test_ring_forward_routes_joint_calls_by_the_setting(monkeypatch):
    """_compact_ring_fwd: with `joint` unset a joint call never reaches the steady layer; under "steady" it does when the layer matches
    and the pair agrees with q - as a trailing POSITIONAL argument of `run` -, the malformed pairs raise what the general path raises, and
    a pair that disagrees with q takes the general path"""
    import compactfusion_amd
    from compactfusion_amd import config
    from compactfusion_amd.compact import ring as R

    class Stop(Exception):
        pass

    class St:
        def matches(self, *a):
            return True

        def run(self, *a):
            ran.append(a)
            return "steady"
    ran = []
    q = torch.zeros(1, 9, 2, 16, dtype=torch.float16)
    k = v = torch.zeros(1, 6, 2, 16, dtype=torch.float16)
    jk, jv = torch.zeros(1, 3, 2, 16, dtype=torch.float16), torch.ones(1, 3, 2, 16, dtype=torch.float16)

    class Cfg:
        compress_func = staticmethod(lambda l, s: None)
    monkeypatch.setattr(R, "compact_config", lambda: Cfg)
    monkeypatch.setattr(R, "RingComm", lambda g: (_ for _ in ()).throw(Stop()))          # the general path's first step
    monkeypatch.setitem(R._steady, (7, None), St())
    fwd = lambda **kw: R._compact_ring_fwd(q, k, v, causal=False, mod_idx=7, current_iter=3, **kw)      # noqa: E731
    config.reset()
    try:
        monkeypatch.delenv("CFX_JOINT", raising=False)
        assert fwd() == "steady" and len(ran[-1]) == 4
        with pytest.raises(Stop):
            fwd(joint_tensor_key=jk, joint_tensor_value=jv, joint_strategy="front")
        assert len(ran) == 1
        compactfusion_amd.configure(joint="steady")
        assert fwd() == "steady" and len(ran[-1]) == 4
        for strategy in ("front", "rear"):
            assert fwd(joint_tensor_key=jk, joint_tensor_value=jv, joint_strategy=strategy) == "steady"
            a = ran[-1]
            assert len(a) == 5 and a[0] is q and a[4][0] is jk and a[4][1] is jv and a[4][2] == strategy
        n = len(ran)
        with pytest.raises(ValueError, match="simultaneously"):
            fwd(joint_tensor_key=jk, joint_strategy="front")
        with pytest.raises(ValueError, match="not supprted"):
            fwd(joint_tensor_key=jk, joint_tensor_value=jv, joint_strategy="none")
        for bad_k, bad_v in ((jk.float(), jv.float()), (jk[:, :, :1], jv[:, :, :1]), (jk, jv[:, :2]), (jk[..., :8], jv[..., :8])):
            with pytest.raises(Stop):
                fwd(joint_tensor_key=bad_k, joint_tensor_value=bad_v, joint_strategy="rear")
        assert len(ran) == n
    finally:
        config.reset()
