"""The native attention forward over all of a layer's K,V blocks (cfx_attn_fwd_blocks, attention_blocks, configure(attention=...)) on the
CPU: the eager fallback against the float64 witness and derived bound of tests/_attn_f64.py on every case of tests/_attn_cases.py;
planted errors, each at least 10 x the bound on every case that can show it; the single key bit for bit; the C-ABI's argument checks;
the setting; the calls `_blocks` makes; the new source's resource rows.  No GPU."""
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

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c["id"] for c in C.CASES]
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
_refs = {}


def ref_of(case, dtype):
    """the case's inputs and its witness / bound, computed once"""
    key = (case["id"], dtype)
    if key not in _refs:
        q, ks, vs, scale = C.build(case, dtype)
        _refs[key] = (q, ks, vs, scale, W.reference_and_bound(q, ks, vs, scale, dtype))
    return _refs[key]


def test_case_list_covers_what_it_claims():
    cs = C.CASES
    assert 35 <= len(cs) <= 45 and len(set(IDS)) == len(cs)
    assert {c["Sq"] for c in cs} == set(C.SQS) and {c["Sk"] for c in cs} == set(C.SKS) and {c["n"] for c in cs} == set(C.NS)
    assert {c["H"] for c in cs} == {1, 3} and {c["B"] for c in cs} == {1, 2} and {c["D"] for c in cs} == {64, 128}
    assert {c["kind"] for c in cs} == {"gauss", "int", "peak", "ramp", "vmax", "zeroq", "equal"}
    assert {c["where"] for c in cs if c["kind"] == "peak"} == {"tile_first", "tile_last", "block_last", "tail", "lastblock_first"}
    for dtype in TDT:
        for c in cs:
            q, ks, vs, scale, (ro, rl, ob, lb) = ref_of(c, dtype)
            if c["kind"] == "peak":                                  # the designated key carries more than 0.9 of every row
                s, _ = W.scores(q, ks, scale)
                blk, key = C.peak_position(c)
                w = np.exp(s - rl.transpose(0, 2, 1)[..., None])
                assert w[..., blk * c["Sk"] + key].min() > 0.9, c["id"]
            if c["kind"] == "ramp":                                  # scores reach +-1e4 where the ramp has that many blocks
                s, _ = W.scores(q, ks, scale)
                assert s.max() > (9000 if c["n"] >= 3 else 25) and (s.min() < -9000 or c["n"] < 4), c["id"]
        top = {"fp16": 65504.0, "bf16": 2.0 ** 100}[dtype]
        assert all(np.abs(ref_of(c, dtype)[2][0]).max() == top for c in cs if c["kind"] == "vmax")


@pytest.mark.parametrize("dtype", list(TDT))
@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_eager_fallback_meets_the_bound(case, dtype, monkeypatch):
    from compactfusion_amd.compact import attention as A
    monkeypatch.setattr(A, "_attn_fwd_native", lambda *a, **k: pytest.fail("CPU tensors reached the native launch"))
    q, ks, vs, scale, ref = ref_of(case, dtype)
    t = lambda x: torch.from_numpy(x).to(TDT[dtype])       # noqa: E731
    tq, tks, tvs = t(q), [t(k) for k in ks], [t(v) for v in vs]
    assert torch.equal(tq.float(), torch.from_numpy(q))
    out, lse = A.attention_blocks(tq, tks, tvs, scale)
    B, Sq, H, D = q.shape
    assert out.dtype == TDT[dtype] and tuple(out.shape) == (B, Sq, H, D) and out.is_contiguous()
    assert lse.dtype == torch.float32 and tuple(lse.shape) == (B, H, Sq) and lse.stride() == (Sq * H, 1, H)
    fo, fl = W.check(out.float().numpy(), lse.transpose(1, 2).numpy(), ref, "attention_blocks, eager fallback")
    print(f"{case['id']} {dtype}: eager fallback {fo:.3f} / {fl:.3f} of the bound (out / lse)")
    if case["D"] == 64 and case["n"] <= 3:                 # the default scale is D ** -0.5
        o2, l2 = A.attention_blocks(tq, tks, tvs)
        assert torch.equal(o2, out) and torch.equal(l2, lse)


def test_eager_fallback_refusals():
    from compactfusion_amd.compact import attention as A
    q = torch.zeros(1, 2, 1, 64, dtype=torch.float16)
    with pytest.raises(ValueError):
        A.attention_blocks(q, [], [])
    with pytest.raises(ValueError):
        A.attention_blocks(q, [q, q], [q])
    out, lse = A.attention_blocks(q, [q] * 20, [q] * 20)                 # more than 16 blocks: the eager path takes any number
    assert tuple(out.shape) == (1, 2, 1, 64) and torch.allclose(lse, torch.full_like(lse, float(np.log(40.0))))
    assert not A.attn_native_ok(q, [q], [q])


@pytest.mark.parametrize("dtype", list(TDT))
@pytest.mark.parametrize("plant", W.PLANTS)
def test_planted_errors_exceed_the_bound_tenfold(plant, dtype):
    """per case: every case whose shape and values can show the error (W.can_show: decided from the case alone) does, by 10 x the
    bound on at least one element of out or lse - so the GPU test's pass on these cases is not vacuous"""
    shown = 0
    for c in C.CASES:
        if not W.can_show(plant, c):
            continue
        q, ks, vs, scale, ref = ref_of(c, dtype)
        fo, fl = W.excess(*W.planted(plant, q, ks, vs, scale), ref)
        assert max(fo, fl) >= 10.0, f"{plant} on {c['id']} {dtype}: only {fo:.2f} / {fl:.2f} x the bound (out / lse)"
        shown += 1
    assert shown >= 5, f"{plant}: only {shown} cases can show it"


@pytest.mark.parametrize("dtype", list(TDT))
def test_the_witness_itself_is_inside_its_bound_and_exact_on_a_single_key(dtype):
    case = next(c for c in C.CASES if c["kind"] == "int" and c["Sk"] == 1 and c["Sq"] > 1)
    q, ks, vs, scale, ref = ref_of(case, dtype)
    ro, rl = ref[0], ref[1]
    assert np.array_equal(ro, np.broadcast_to(vs[0].astype(np.float64), ro.shape))          # n = 1, Sk = 1: out == v ...
    dot = np.einsum("bqhd,bkhd->bqh", q.astype(np.float64), ks[0].astype(np.float64))
    assert np.array_equal(rl, float(np.float32(scale)) * dot)                                # ... and lse == scale q.k
    assert W.check(ro, rl, ref) == (0.0, 0.0)
    from compactfusion_amd.compact import attention as A
    t = lambda x: torch.from_numpy(x).to(TDT[dtype])       # noqa: E731
    out, lse = A.attention_blocks(t(q), [t(ks[0])], [t(vs[0])], scale)
    assert torch.equal(out, t(vs[0]).expand_as(out))                                         # the eager fallback: the same bits
    assert np.array_equal(lse.transpose(1, 2).numpy(), (np.float32(scale) * dot.astype(np.float32)).astype(np.float32))


def test_c_abi_argument_checks_without_a_gpu():
    """every argument error, in the documented order: NULL, flag bits, n / shape / scale, alignment (a pending gate error needs a
    device).  Each returns before any launch: the context's launch count stays 0."""
    from compactfusion_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(REPO, "include", "cfx.h")).read()
    assert re.search(r"\bint cfx_attn_fwd_blocks\(cfx_ctx\* ctx, int n, const void\* q, const void\* const\* ks, const void\* const\* vs, "
                     r"int B, int Sq, int Sk, int H, int D,\s+float softmax_scale, unsigned flags, void\* out, void\* lse, void\* stream\);", hdr)
    assert "#define CFX_ATTN_MAX_BLOCKS 16" in hdr and re.search(r"\bint cfx_attn_fwd_launches\(cfx_ctx\* ctx, unsigned long long\* n\);", hdr)
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT cfx_attn_fwd_blocks\b", exported) and re.search(r"\bT cfx_attn_fwd_launches\b", exported)
    assert {"cfx_attn_fwd_blocks", "cfx_attn_fwd_launches"} <= {n for n, _, _ in _lib.SYMBOLS}
    assert _lib.ATTN_MAX_BLOCKS == 16 and lib.cfx_abi_version() == 2
    ctx = lib.cfx_create(0)
    assert ctx
    f = lib.cfx_attn_fwd_blocks
    P = ctypes.c_void_p * 17
    ks = P(*[0x10000 + 0x1000 * i for i in range(17)])
    vs = P(*[0x40000 + 0x1000 * i for i in range(17)])
    q, out, lse = 0x70000, 0x80000, 0x90000
    NULL, SHAPE, ALIGN, CODEC = -1, -2, -3, -4
    BF = _lib.ELEM_BF16

    def count():
        n = ctypes.c_ulonglong(99)
        assert lib.cfx_attn_fwd_launches(ctx, ctypes.byref(n)) == 0
        return n.value
    assert count() == 0
    assert lib.cfx_attn_fwd_launches(None, ctypes.byref(ctypes.c_ulonglong())) == NULL and lib.cfx_attn_fwd_launches(ctx, None) == NULL
    # 1. NULL pointers, table entries included - before anything else
    assert f(None, 2, q, ks, vs, 1, 4, 4, 2, 64, 0.125, 0, out, lse, None) == NULL
    assert f(ctx, 2, None, ks, vs, 1, 4, 4, 2, 64, 0.125, 0, out, lse, None) == NULL
    assert f(ctx, 2, q, None, vs, 1, 4, 4, 2, 64, 0.125, 0, out, lse, None) == NULL
    assert f(ctx, 2, q, ks, None, 1, 4, 4, 2, 64, 0.125, 0, out, lse, None) == NULL
    assert f(ctx, 2, q, ks, vs, 1, 4, 4, 2, 64, 0.125, 0, None, lse, None) == NULL
    assert f(ctx, 2, q, ks, vs, 1, 4, 4, 2, 64, 0.125, 0, out, None, None) == NULL
    assert b"null" in lib.cfx_last_error_string(ctx)
    for k in (0, 1, 15):
        holed = P(*[None if i == k else 0x10000 + 0x1000 * i for i in range(17)])
        assert f(ctx, 16, q, holed, vs, 1, 4, 4, 2, 64, 0.125, 0, out, lse, None) == NULL
        assert f(ctx, 16, q, ks, holed, 1, 4, 4, 2, 64, 0.125, 0, out, lse, None) == NULL
        assert f(ctx, 16, q, holed, vs, 1, 4, 4, 2, 20, -1.0, 0x40, 0x80002, lse, None) == NULL      # ... whatever else is wrong
    holed = P(*[None if i == 3 else 0x10000 + 0x1000 * i for i in range(17)])
    assert f(ctx, 3, q, holed, vs, 1, 4, 4, 2, 64, 0.125, 0x40, out, lse, None) == CODEC                  # (entry 3 is not one of 3 blocks)
    # 2. flag bits: CFX_ELEM_BF16 only
    for bad in (1, 2, 4, 0x40, 0x200, BF | 1, 0xFFFFFFFF):
        assert f(ctx, 2, q, ks, vs, 1, 4, 4, 2, 64, 0.125, bad, out, lse, None) == CODEC, bad
        assert f(ctx, 0, q, ks, vs, 1, 4, 4, 2, 20, 0.0, bad, 0x80002, lse, None) == CODEC            # ... before n, the shape and the alignment
    assert b"flag" in lib.cfx_last_error_string(ctx)
    # 3. n outside 1 .. 16, the sizes, the head dim, the launch's size, the scale
    for fl in (0, BF):
        for n in (0, 17, -1, 1 << 20):
            assert f(ctx, n, q, ks, vs, 1, 4, 4, 2, 64, 0.125, fl, 0x80002, lse, None) == SHAPE, (fl, n)
        for B, Sq, Sk, H, D in ((0, 4, 4, 2, 64), (1, 0, 4, 2, 64), (1, 4, 0, 2, 64), (1, 4, 4, 0, 64), (-1, 4, 4, 2, 64), (1, 4, 4, 2, 0),
                                (1, 4, 4, 2, 32), (1, 4, 4, 2, 96), (1, 4, 4, 2, 256), (1, 4, 4, 2, -64),
                                (1 << 20, 1 << 20, 4, 1 << 10, 64)):                           # 2^20 x 2^13 x 2^10 workgroups
            assert f(ctx, 2, q, ks, vs, B, Sq, Sk, H, D, 0.125, fl, 0x80002, lse, None) == SHAPE, (B, Sq, Sk, H, D)
        for sc in (0.0, -0.125, float("inf"), float("-inf"), float("nan")):
            assert f(ctx, 2, q, ks, vs, 1, 4, 4, 2, 64, sc, fl, 0x80002, lse, None) == SHAPE, sc
    # 4. 16-byte alignment of q, out, lse and of every block
    for bq, bo, bl in ((q + 2, out, lse), (q, out + 8, lse), (q, out, lse + 4)):
        assert f(ctx, 2, bq, ks, vs, 1, 4, 4, 2, 64, 0.125, 0, bo, bl, None) == ALIGN
    for k in (0, 7, 15):
        off = P(*[0x10000 + 0x1000 * i + (2 if i == k else 0) for i in range(17)])
        assert f(ctx, 16, q, off, vs, 1, 4, 4, 2, 64, 0.125, BF, out, lse, None) == ALIGN
        assert f(ctx, 16, q, ks, off, 1, 4, 4, 2, 64, 0.125, 0, out, lse, None) == ALIGN
    assert count() == 0
    # the query-tile setter: 0 (the library's choice), 64, 128, 256
    assert "cfx_set_attn_qtile" in {n for n, _, _ in _lib.SYMBOLS} and re.search(r"\bint cfx_set_attn_qtile\(cfx_ctx\* ctx, int rows\);", hdr)
    assert [lib.cfx_set_attn_qtile(ctx, r) for r in (64, 128, 256, 0)] == [0] * 4 and lib.cfx_set_attn_qtile(None, 64) == NULL
    assert [lib.cfx_set_attn_qtile(ctx, r) for r in (32, 96, 512, -64, 1)] == [SHAPE] * 5
    lib.cfx_destroy(ctx)


def test_resource_rows_of_the_new_source():
    """cfx_attn.hip alone: the twelve k_attn_fwd_blocks instantiations (2 element types x 2 head dims x 3 query tiles) plus the
    k_copy_probe cfx_device.h puts in every translation unit; no scratch; VGPRs + AGPRs at most 512; LDS at most the 64 KiB a workgroup
    may declare statically - and what profiles/attn_native_rows.json records is what the compiler reports.  The source sits in a list of
    its own, beside SRC, CAPTURE_SRC and MERGE_SRC."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import resource_usage as RU
    finally:
        sys.path.pop(0)
    from compactfusion_amd import build as B
    assert [os.path.basename(p) for p in B.ATTN_SRC] == ["cfx_attn.hip"]
    assert not set(B.ATTN_SRC) & (set(B.SRC) | set(B.CAPTURE_SRC) | set(B.MERGE_SRC))
    rows = RU._one(B.ATTN_SRC[0])
    names = [re.sub(r"^void ", "", re.sub(r"\(.*$", "", d)) for d in RU.demangle([r["name"] for r in rows])]
    want = [f"k_attn_fwd_blocks<{e}, {d}, {nw}>" for e in ("ElemF16", "ElemBF16") for d in (64, 128) for nw in (2, 4, 8)]
    assert sorted(names) == sorted(["k_copy_probe"] + want), names
    found = {}
    for r, name in zip(rows, names):
        assert r.get("scratch", 0) == 0, (name, r)
        assert r.get("vgpr", 0) + r.get("agpr", 0) <= 512, (name, r)
        if name != "k_copy_probe":
            d = int(name.split(",")[1])
            assert r.get("lds", 0) == 4 * 64 * d * 2 <= 65536, (name, r)              # two K and two V tiles of 64 keys
            found[name] = {k: r.get(k, 0) for k in ("vgpr", "agpr", "sgpr", "scratch", "lds", "occupancy")}
    recorded = json.load(open(os.path.join(REPO, "profiles", "attn_native_rows.json")))["resource_rows"]
    assert recorded == found, "profiles/attn_native_rows.json: resource_rows differ from what the compiler reports (tools/attn_rows.py --resources rewrites them)"
    import inspect
    assert "ATTN_SRC" in inspect.getsource(B.needs_build) and "ATTN_SRC" in inspect.getsource(B.build_lib)      # built into, and a dependency of, both libraries


def test_configure_attention(monkeypatch):
    import compactfusion_amd
    from compactfusion_amd import config
    config.reset()
    try:
        monkeypatch.delenv("CFX_ATTENTION", raising=False)
        assert config.get("attention") == "sdpa" and compactfusion_amd.configure()["attention"] == "sdpa"
        monkeypatch.setenv("CFX_ATTENTION", "native")
        assert config.get("attention") == "native"
        assert compactfusion_amd.configure(attention="sdpa")["attention"] == "sdpa"              # an explicit configure() overrides it
        assert compactfusion_amd.configure(attention="native")["attention"] == "native"
        with pytest.raises(ValueError):
            compactfusion_amd.configure(attention="flash")
        assert config.get("attention") == "native"
        config.reset()
        monkeypatch.setenv("CFX_ATTENTION", "both")
        with pytest.raises(ValueError):
            config.get("attention")
    finally:
        config.reset()
    assert "CFX_ATTENTION" in config.__doc__ and "attn_merge is ignored" in config.__doc__
    assert "CFX_ATTENTION" in open(os.path.join(REPO, "INTEGRATION.md")).read()


# ---- _blocks on CPU stand-ins: which calls the native mode makes ----------------------------------------------------------------------
WR, SHAPE = 4, (1, 6, 2, 16)


@pytest.fixture
def layer(monkeypatch):
    """a steady layer of WR ranks with CPU tensors for its peers' states; a stand-in for the launch (the eager definition) and spies on
    everything compact/ring.py calls around it"""
    from compactfusion_amd import config
    from compactfusion_amd.compact import attention as A
    from compactfusion_amd.compact import ring as R
    g = torch.Generator().manual_seed(11)
    q, k, v = (torch.randn(SHAPE, generator=g).to(torch.float16) for _ in range(3))
    peers = [(s, torch.randn(SHAPE, generator=g).to(torch.float16), torch.randn(SHAPE, generator=g).to(torch.float16)) for s in range(1, WR)]
    st = R._SteadyLayer.__new__(R._SteadyLayer)
    st.world, st._peers, st._fast = WR, peers, False
    calls = []
    backend = {"ok": True}

    def launch(q_, ks, vs, scale, tabs=None):
        calls.append(("launch", (q_, list(ks), list(vs), scale, tabs)))
        return A.attention_blocks(q_, ks, vs, scale)                 # CPU tensors: the eager definition

    def spied(name, fn):
        def wrap(*a, **kw):
            calls.append((name, a))
            return fn(*a, **kw)
        return wrap
    monkeypatch.setattr(R, "attn_native_ok", lambda q_, ks, vs: backend["ok"])
    monkeypatch.setattr(R, "_attn_fwd_native", launch)
    monkeypatch.setattr(R, "merge_blocks", spied("merge_blocks", A.merge_blocks))
    monkeypatch.setattr(R, "update_out_and_lse", spied("update_out_and_lse", A.update_out_and_lse))
    monkeypatch.setattr(R, "block_attention", spied("block_attention", A.block_attention))
    monkeypatch.setattr(R, "flag_wait", lambda wait, device: calls.append(("flag_wait", wait)))
    monkeypatch.setattr(A, "flag_wait", lambda wait, device: calls.append(("flag_wait(in merge)", wait)))
    config.reset()
    yield st, q, k, v, peers, calls, backend
    config.reset()


@pytest.mark.parametrize("merge", ["chain", "once"])
@pytest.mark.parametrize("lane", [False, True])
def test_blocks_native_makes_one_launch_behind_the_chain_and_its_waits(layer, lane, merge):
    import compactfusion_amd
    st, q, k, v, peers, calls, backend = layer
    order = []
    flagf = lambda r: 0x1000 + 64 * r        # noqa: E731
    args = (lambda s, lean: (order.append(("issue", s, lean)), calls.append(("issue", (s, lean)))), flagf, 5) if lane else ()
    scale = q.shape[-1] ** -0.5
    compactfusion_amd.configure(attention="sdpa", attn_merge=merge)
    want = st._blocks(q, k, v, scale, None, *args)
    assert "launch" not in [c[0] for c in calls]
    del calls[:], order[:]
    compactfusion_amd.configure(attention="native")                  # attn_merge stays what it was: ignored
    got = st._blocks(q, k, v, scale, None, *args)
    names = [c[0] for c in calls]
    if lane:        # the whole chain first, in block order; then a stand-alone wait per peer flag; then the one launch
        assert names == ["issue"] * WR + ["flag_wait"] * (WR - 1) + ["launch"], names
        assert [c[1] for c in calls[:WR]] == [(s, True) for s in range(WR)]
        assert [c[1] for c in calls[WR:2 * WR - 1]] == [(flagf(s), 5) for s in range(1, WR)]
    else:
        assert names == ["launch"], names
    lq, lks, lvs, lscale, tabs = calls[-1][1]
    assert lq is q and lscale == scale and len(lks) == len(lvs) == WR
    assert lks[0] is k and lvs[0] is v and all(a is b for a, (_, b, _) in zip(lks[1:], peers)) and all(a is b for a, (_, _, b) in zip(lvs[1:], peers))
    assert [p for p in tabs[0]] == [t.data_ptr() for t in lks] and [p for p in tabs[1]] == [t.data_ptr() for t in lvs]     # the cached tables, entry 0 this call's
    k2, v2 = k.clone(), v.clone()                                    # another call's K, V: the same table objects, entry 0 rewritten
    st._blocks(q, k2, v2, scale, None, *args)
    assert calls[-1][1][4] is tabs and tabs[0][0] == k2.data_ptr() and tabs[1][0] == v2.data_ptr() and tabs[0][1] == peers[0][1].data_ptr()
    # what is returned has the chain's types, shapes and strides, and is the same attention
    assert got[2] is None and want[2] is None
    for a, b in zip(got[:2], want[:2]):
        assert a.dtype == b.dtype and a.shape == b.shape
    B_, S_, H_, D_ = SHAPE                                           # ... in the layouts the lean loop returns on the GPU (this CPU stand-in's
    assert got[0].is_contiguous() and got[1].stride() == (S_ * H_, 1, H_)      # eager chain has its own; tests/test_gpu_attn_fwd.py compares the real ones)
    assert torch.allclose(got[0].float(), want[0].float(), atol=2e-3, rtol=2e-3) and torch.allclose(got[1], want[1], atol=1e-4, rtol=1e-5)


@pytest.mark.parametrize("merge", ["chain", "once"])
def test_blocks_native_falls_back_to_todays_path(layer, merge):
    """what the launch cannot take (here: the stand-in says no) keeps the path attn_merge names, call for call"""
    import compactfusion_amd
    st, q, k, v, peers, calls, backend = layer
    scale = q.shape[-1] ** -0.5
    compactfusion_amd.configure(attention="sdpa", attn_merge=merge)
    want = st._blocks(q, k, v, scale, None)
    today = [c[0] for c in calls]
    assert today == (["block_attention", "update_out_and_lse"] * WR if merge == "chain" else ["block_attention"] * WR + ["merge_blocks"])
    del calls[:]
    backend["ok"] = False
    compactfusion_amd.configure(attention="native")
    got = st._blocks(q, k, v, scale, None)
    assert [c[0] for c in calls] == today
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # the peers are asked once per layer; this call's own q, k, v every time
    st2 = type(st).__new__(type(st))
    st2.world, st2._peers, st2._fast = 17, peers * 6, False          # more blocks than a launch takes: never native
    backend["ok"] = True
    del calls[:]
    assert st2._native_ok(q, k, v) is False
