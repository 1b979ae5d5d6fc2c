"""The three one-launch attention entry points on the GPU (-m gpu) over the cases of tests/_attn_domain_cases.py: softmax scales that are
not D ** -0.5 - two of them no power of two, 2^-20, 4.0 and the smallest subnormal -, the value kinds vmax / zeroq / equal / int on the
unequal-length walks, and query counts on and around the whole query tiles.  Every case against the float64 witness and the derived
bound of tests/_attn_f64.py / tests/_attn_var_f64.py in ONE counted launch; the two bit-for-bit bridges between the walks at every scale;
the single key's and the zero query's bit identities; every query tile's bits, a row's bits whatever the launch's Sq, guard rows around
out and lse; `attention_blocks` and compact_fwd's steady layer at a caller's scale of 0.3.  A launch, or a Python route, that used
D ** -0.5 for the scale it is given fails every scale test here (tests/test_attn_domain_f64.py: by 1e4 bounds)."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import _attn_cases as C
import _attn_domain_cases as DC
import _attn_f64 as W
import _attn_var_f64 as VW

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _harness():
    """tests/test_gpu_attn_var.py's helpers and its loop-back harness for compact_fwd on the steady layer (`_run_steps`), as a module
    object of this file's own: its shapes and its scale are set below, and the test module pytest collects keeps its own"""
    spec = importlib.util.spec_from_file_location("_attn_var_harness_domain", os.path.join(HERE, "test_gpu_attn_var.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TV = _harness()
BF = 0x100
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
GUARD = 32                                   # guard rows on either side of out and lse: a wave's 32 rows
_lib_ctx, _dev, _count, _outs, _same_bits = TV._lib_ctx, TV._dev, TV._count, TV._outs, TV._same_bits
_refs = {}


def bound_of(case):
    return W.reference_and_bound if case["ep"] == "eq" else VW.reference_and_bound


def ref_of(case, dtype):
    """the case's inputs and its witness / bound, computed once and left unchanged"""
    key = (case["id"], dtype)
    if key not in _refs:
        q, ks, vs, scale = DC.build(case, dtype)
        _refs[key] = (q, ks, vs, scale, bound_of(case)(q, ks, vs, scale, dtype))
    return _refs[key]


def _launch(lib, ctx, ep, q, ks, vs, scale, out=None, lse=None):
    """the entry point `ep` through the C-ABI: cfx_attn_fwd_blocks ("eq"), cfx_attn_fwd_blocks_var ("var"), cfx_attn_fwd_blocks_hd ("hd")"""
    B, Sq, H, D = q.shape
    n = len(ks)
    assert q.is_contiguous() and all(k.is_contiguous() and v.is_contiguous() and k.shape == v.shape and (k.shape[0], k.shape[2], k.shape[3]) == (B, H, D)
                                     for k, v in zip(ks, vs))
    if out is None:
        out, lse = _outs(q)
    assert tuple(out.shape) == (B, Sq, H, D) and tuple(lse.shape) == (B, Sq, H) and out.is_contiguous() and lse.is_contiguous()
    P = ctypes.c_void_p * n
    pk, pv = P(*[t.data_ptr() for t in ks]), P(*[t.data_ptr() for t in vs])
    fl = BF if q.dtype == torch.bfloat16 else 0
    sh = torch.cuda.current_stream().cuda_stream
    if ep == "eq":
        assert all(k.shape == ks[0].shape for k in ks)
        rc = lib.cfx_attn_fwd_blocks(ctx, n, q.data_ptr(), pk, pv, B, Sq, ks[0].shape[1], H, D, scale, fl, out.data_ptr(), lse.data_ptr(), sh)
    else:
        fn = lib.cfx_attn_fwd_blocks_var if ep == "var" else lib.cfx_attn_fwd_blocks_hd
        rc = fn(ctx, n, q.data_ptr(), pk, pv, (ctypes.c_int * n)(*[t.shape[1] for t in ks]), B, Sq, H, D, scale, fl, out.data_ptr(), lse.data_ptr(), sh)
    assert rc == 0, (ep, scale, lib.cfx_last_error_string(ctx))
    return out, lse


def _to_dev(q, ks, vs, dtype):
    return _dev(q, dtype), [_dev(k, dtype) for k in ks], [_dev(v, dtype) for v in vs]


def _every_case(ep, dtype):
    """every scale, kind and single-key case of the entry point: rc 0 (the smallest subnormal scale included), ONE counted launch, out and
    lse within the derived bound of the float64 witness AT THE SCALE PASSED.  One key (sks = [1]): out is v's bits and lse is, bit for
    bit, fp32(a * scale) with a the exact integer sum - at D ** -0.5 and at fp32(0.3).  Prints the largest fraction of the bound per scale."""
    lib, ctx = _lib_ctx()
    worst = {}
    cases = [c for c in DC.of(ep, dtype=dtype) if c["group"] != "sq"]
    assert {c["sname"] for c in cases} >= set(DC.SCALE_NAMES) | {"sub"}
    for case in cases:
        q, ks, vs, scale, ref = ref_of(case, dtype)
        dq, dks, dvs = _to_dev(q, ks, vs, dtype)
        n0 = _count(lib, ctx)
        out, lse = _launch(lib, ctx, ep, dq, dks, dvs, scale)
        torch.cuda.synchronize()
        assert _count(lib, ctx) == n0 + 1, case["id"]
        fo, fl = W.check(out.float().cpu().numpy(), lse.cpu().numpy(), ref, f"{case['id']} {dtype}")
        key = case["sname"] if case["group"] == "scale" else case["group"]
        worst[key] = tuple(max(a, b) for a, b in zip(worst.get(key, (0.0, 0.0)), (fo, fl)))
        if case["group"] == "int" and DC.lengths(case) == [1]:
            assert _same_bits(out, dvs[0].expand_as(out).contiguous()), case["id"]
            a = (q.astype(np.float64)[:, :, :, :] * ks[0].astype(np.float64)).sum(-1)               # (B, Sq, H), exact
            want = np.float32(a) * np.float32(scale)                                                # ONE fp32 rounding
            assert want.dtype == np.float32 and np.array_equal(np.float32(a).astype(np.float64), a)
            assert np.array_equal(lse.cpu().numpy().view(np.uint32), want.view(np.uint32)), f"{case['id']}: lse is not fp32(a * scale) bit for bit"
    assert lib.cfx_gate_errors(ctx) == 0
    for key, (fo, fl) in worst.items():
        print(f"{ep} {dtype} {key}: {fo:.3f} / {fl:.3f} of the bound (out / lse)")


def test_every_case_within_witness_and_bound_in_one_launch():
    """all cases of every entry point and element type (ONE test: a case is milliseconds of GPU work, and a miss names its case)"""
    for ep in DC.ENTRIES:
        for dtype in TDT:
            _every_case(ep, dtype)


def _bridges(dtype):
    """at EVERY scale of the list (and peak, ramp, the subnormal): cfx_attn_fwd_blocks_var on blocks of one length returns
    cfx_attn_fwd_blocks's bits, and cfx_attn_fwd_blocks_hd returns the bits of cfx_attn_fwd_blocks_var on q and the blocks zero-padded
    to D = 128 with the same scale - so the three copies of the walk make the scale product the same way"""
    lib, ctx = _lib_ctx()
    seen = set()
    for case in DC.of("eq", "scale", dtype):
        q, ks, vs, scale, _ = ref_of(case, dtype)
        dq, dks, dvs = _to_dev(q, ks, vs, dtype)
        o0, l0 = _launch(lib, ctx, "eq", dq, dks, dvs, scale)
        o1, l1 = _launch(lib, ctx, "var", dq, dks, dvs, scale)
        torch.cuda.synchronize()
        assert _same_bits(o1, o0) and _same_bits(l1, l0), case["id"]
        seen.add(("eq", case["sname"]))
    for case in DC.of("hd", "scale", dtype):
        q, ks, vs, scale, _ = ref_of(case, dtype)
        D = case["D"]
        dq, dks, dvs = _to_dev(q, ks, vs, dtype)
        pad = lambda t: torch.nn.functional.pad(t, (0, 128 - D)).contiguous()           # noqa: E731
        o1, l1 = _launch(lib, ctx, "hd", dq, dks, dvs, scale)
        o0, l0 = _launch(lib, ctx, "var", pad(dq), [pad(k) for k in dks], [pad(v) for v in dvs], scale)
        torch.cuda.synchronize()
        assert _same_bits(o1, o0[..., :D].contiguous()) and _same_bits(l1, l0), case["id"]
        assert not o0[..., D:].any()
        seen.add(("hd", case["sname"]))
    assert seen == {(ep, s) for ep in ("eq", "hd") for s in DC.SCALE_NAMES + ("sub",)}


def _zero_queries(dtype):
    """q = 0: a_j = 0 and 0 * scale = 0 whatever the scale, so out and lse are the default scale's bits at every scale of the list -
    every zeroq case of the unequal-length walks, and the equal launch's own two"""
    lib, ctx = _lib_ctx()
    runs = [(c["ep"], c, DC.build(c, dtype)) for c in DC.of(group="kind", dtype=dtype, kind="zeroq")]
    runs += [("eq", c, C.build(c, dtype)) for c in C.CASES if c["kind"] == "zeroq"]
    assert len(runs) == 3 * 5 + 2
    for ep, case, (q, ks, vs, scale) in runs:
        assert scale == DC.scale_of("def", case["D"]) and not q.any()
        dq, dks, dvs = _to_dev(q, ks, vs, dtype)
        out, lse = _launch(lib, ctx, ep, dq, dks, dvs, scale)
        for sname in DC.SCALE_NAMES:
            o, l = _launch(lib, ctx, ep, dq, dks, dvs, DC.scale_of(sname, case["D"]))
            torch.cuda.synchronize()
            assert _same_bits(o, out) and _same_bits(l, lse), (case["id"], sname)
        bound = bound_of(dict(ep=ep))(q, ks, vs, scale, dtype)
        W.check(out.float().cpu().numpy(), lse.cpu().numpy(), bound, f"{case['id']} {dtype}")


def test_bridges_and_zero_queries_hold_at_every_scale():
    """the two bit-for-bit bridges between the walks (`_bridges`) and the zero query's bits (`_zero_queries`), fp16 and bf16"""
    for dtype in TDT:
        _bridges(dtype)
        _zero_queries(dtype)


def _guarded(B, Sq, H, D, dtype):
    """out (B, Sq, H, D) and lse (B, Sq, H) as the middle of NaN-filled buffers with GUARD rows in front and behind (B = 1: contiguous)"""
    assert B == 1
    ob = torch.full((1, Sq + 2 * GUARD, H, D), float("nan"), dtype=dtype, device="cuda")
    lb = torch.full((1, Sq + 2 * GUARD, H), float("nan"), dtype=torch.float32, device="cuda")
    out, lse = ob[:, GUARD:GUARD + Sq], lb[:, GUARD:GUARD + Sq]
    assert out.is_contiguous() and lse.is_contiguous() and out.data_ptr() % 16 == 0 and lse.data_ptr() % 16 == 0
    return ob, lb, out, lse


def _guards_intact(ob, lb, Sq):
    return bool(torch.isnan(ob[:, :GUARD]).all() and torch.isnan(ob[:, GUARD + Sq:]).all() and torch.isnan(lb[:, :GUARD]).all()
                and torch.isnan(lb[:, GUARD + Sq:]).all())


def _query_counts(ep, D, dtype):
    """Sq = 31 .. 257 (fp16; bf16 at 128 and 256): where nqt = ceil(Sq / qtile) and a wave's `q0 < Sq` sit on their boundary for the
    three query tiles.  Each Sq is the q prefix of ONE 257-row case over the same blocks.  Per Sq: one counted launch within the bound; its
    rows ARE the same rows of the 257-row launch, bit for bit (a row's arithmetic depends on no other row - a tail or boundary slip
    breaks this without any tolerance); query tiles 64, 128 and 256 return the library's choice's bits; out and lse lie inside NaN-filled
    buffers whose 32 guard rows on either side stay NaN."""
    lib, ctx = _lib_ctx()
    cases = DC.of(ep, "sq", dtype, D=D)
    assert [c["Sq"] for c in cases] == (list(DC.SQS) if dtype == "fp16" else [128, 256, 257])
    q, ks, vs, scale, ref = ref_of(DC.sq_base(cases[0]), dtype)
    dq, dks, dvs = _to_dev(q, ks, vs, dtype)
    top_out, top_lse = _launch(lib, ctx, ep, dq, dks, dvs, scale)
    torch.cuda.synchronize()
    W.check(top_out.float().cpu().numpy(), top_lse.cpu().numpy(), ref, f"{ep} d{D} {dtype}, 257 rows")
    try:
        for case in cases:
            Sq = case["Sq"]
            qs = dq[:, :Sq]
            assert qs.is_contiguous() and np.array_equal(DC.build(case, dtype)[0], q[:, :Sq])
            got = {}
            for rows in (0, 64, 128, 256):
                assert lib.cfx_set_attn_qtile(ctx, rows) == 0
                ob, lb, out, lse = _guarded(1, Sq, case["H"], D, TDT[dtype])
                n0 = _count(lib, ctx)
                _launch(lib, ctx, ep, qs, dks, dvs, scale, out, lse)
                torch.cuda.synchronize()
                assert _count(lib, ctx) == n0 + 1
                assert _guards_intact(ob, lb, Sq), f"{case['id']} {dtype}, query tile {rows}: a guard row of out or lse was written"
                got[rows] = (out.clone(), lse.clone())
                assert _same_bits(got[rows][0], got[0][0]) and _same_bits(got[rows][1], got[0][1]), (case["id"], rows)
            out, lse = got[0]
            assert torch.isfinite(out).all() and torch.isfinite(lse).all()
            assert _same_bits(out, top_out[:, :Sq].contiguous()) and _same_bits(lse, top_lse[:, :Sq].contiguous()), \
                f"{case['id']} {dtype}: rows differ from the same rows of the 257-row launch"
            W.check(out.float().cpu().numpy(), lse.cpu().numpy(), tuple(r[:, :Sq] for r in ref), f"{case['id']} {dtype}")
    finally:
        assert lib.cfx_set_attn_qtile(ctx, 0) == 0


def test_query_counts_on_and_around_the_whole_tiles():
    """`_query_counts` for the equal launch and var at D 64, hd at D 72 and 120; fp16 at every Sq, bf16 at 128 and 256"""
    for ep, D in DC.SQ_DIMS:
        for dtype in TDT:
            _query_counts(ep, D, dtype)


def _attention_blocks(ep, dtype):
    """attention_blocks(q, ks, vs, 0.3) on the entry point's blocks: ONE launch, within the bound of the witness at fp32(0.3), and the
    bits of the C-ABI launch at that scale"""
    from compactfusion_amd.compact import attention as A
    lib, ctx = _lib_ctx()
    case = DC.of(ep, "scale", dtype, kind="gauss", sname="p3")[0]
    q, ks, vs, scale, ref = ref_of(case, dtype)
    assert scale == float(np.float32(0.3))
    dq, dks, dvs = _to_dev(q, ks, vs, dtype)
    assert A.attn_native_ok(dq, dks, dvs) == (ep == "eq") and A.attn_native_var_ok(dq, dks, dvs)
    n0 = A.attn_fwd_launches(0)
    out, lse = A.attention_blocks(dq, dks, dvs, 0.3)
    torch.cuda.synchronize()
    assert A.attn_fwd_launches(0) == n0 + 1
    W.check(out.float().cpu().numpy(), lse.transpose(1, 2).cpu().numpy(), ref, f"attention_blocks at 0.3, {case['id']} {dtype}")
    o1, l1 = _launch(lib, ctx, ep, dq, dks, dvs, scale)
    torch.cuda.synchronize()
    assert _same_bits(out, o1) and _same_bits(lse.transpose(1, 2).contiguous(), l1)


class _WitnessAt:
    """tests/_attn_var_f64.py as the harness sees it, with the witness and the bound AT ONE SCALE whatever the harness passes"""

    def __init__(self, scale):
        self.scale = scale
        self.check = VW.check

    def reference_and_bound(self, q, ks, vs, scale, dtype):
        return VW.reference_and_bound(q, ks, vs, self.scale, dtype)


def _steady_layer(monkeypatch, D):
    """compact_fwd(..., softmax_scale=0.3), W = 4, configure(joint="steady", attention="native"), heads of 64 (cfx_attn_fwd_blocks
    without joint tensors, cfx_attn_fwd_blocks_var with) and of 72 (cfx_attn_fwd_blocks_hd): tests/test_gpu_attn_var.py's loop-back
    harness with every call given the scale and its witness taken at 0.3.  Every steady call - with joint tensors (steps 3, 5) and
    without (step 4) - is exactly ONE attention launch, no SDPA call, no merge, within the bound of the witness at 0.3 (asserted in the
    harness); the calls before the layer is bound run SDPA at the same scale."""
    from compactfusion_amd.compact import ring
    monkeypatch.setattr(TV, "KV", (1, 64, 8, D))
    monkeypatch.setattr(TV, "QS", (1, 80, 8, D))
    monkeypatch.setattr(TV, "JS", (1, 16, 8, D))
    monkeypatch.setattr(TV, "VW", _WitnessAt(0.3))
    real = ring.compact_fwd
    given = []

    def at_scale(*a, **kw):
        given.append(kw.setdefault("softmax_scale", 0.3))
        return real(*a, **kw)
    monkeypatch.setattr(ring, "compact_fwd", at_scale)
    got = TV._run_steps(monkeypatch, "off", torch.float16, "front", "steady", "native")
    assert given == [0.3] * len(got) and len(got) == (TV.STEPS + 1) * TV.L
    steady = [key for key in sorted(got) if got[key]["steady"]]
    for key in steady:
        b = got[key]
        assert b["attn"] == 1 and b["sdpa"] == 0 and b["merges"] == 0, f"{key}: native made {b['attn']} launches, {b['sdpa']} SDPA calls, {b['merges']} merges"
    assert {(s, l) for s in (3, 4, 5) for l in range(TV.L)} <= set(steady), steady          # joint (3, 5) and plain (4) calls
    assert any(got[k]["joint"] for k in steady) and any(not got[k]["joint"] for k in steady)


def test_python_routes_forward_a_callers_scale(monkeypatch):
    """`attention_blocks` on every entry point's blocks in both element types, and compact_fwd's steady layer at heads of 64 and 72,
    each given softmax_scale = 0.3"""
    for ep in DC.ENTRIES:
        for dtype in TDT:
            _attention_blocks(ep, dtype)
    for D in (64, 72):
        with monkeypatch.context() as m:
            _steady_layer(m, D)
