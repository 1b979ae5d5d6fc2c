"""The one-launch attention's scale, value-kind and query-count cases (tests/_attn_domain_cases.py) on the CPU: the list covers what it
claims; the witness and the bound are the existing ones (tests/_attn_f64.py, tests/_attn_var_f64.py - they carry the scale already, no
new constant); a result computed with ANOTHER scale than the one passed, or with the scale applied to q in the element type, exceeds the
bound tenfold wherever the case can show it - and is exactly the witness where it cannot; one key gained in a tail tile shows in every
flat case; the eager definition of `attention_blocks` honours a caller's scale.  No GPU."""
import numpy as np
import pytest
import torch

import _attn_cases as C
import _attn_domain_cases as DC
import _attn_f64 as W
import _attn_var_f64 as VW

TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
PLANTS = ("defscale", "noscale", "qscaled")
_refs = {}


def bound_of(case):
    """the entry point's own bound: equal lengths _attn_f64's, unequal ones _attn_var_f64's (the same numbers on equal lengths)"""
    return W.reference_and_bound if case["ep"] == "eq" else VW.reference_and_bound


def ref_of(case, dtype):
    """the case's inputs and its witness / bound, computed once and left unchanged"""
    key = (case["id"], dtype)
    if key not in _refs:
        q, ks, vs, scale = DC.build(case, dtype)
        _refs[key] = (q, ks, vs, scale, bound_of(case)(q, ks, vs, scale, dtype))
    return _refs[key]


def can_show(plant, case, dtype):
    """Whether a `scale` case makes the planted error move the result by more than rounding - from the case alone, never from a result.
    defscale  the scale argument ignored for fp32(D ** -0.5): every score is off by the factor scale / D ** -0.5, which is at most 1 / 3
              or at least 2.4 here - a Gaussian row's lse moves by tenths, a peak's or a ramp's by the order of its scores
    noscale   the scores left unscaled: the same, unless the scale IS 1.0 - then it is the witness
    qscaled   q * scale rounded to the element type before the products: exact where the scale is a power of two and q * scale
              neither overflows nor goes subnormal (1.0, 4.0; 2^-20 in bf16 only - fp16's least normal is 2^-14); at fp32(0.3) each
              q_d is off by up to e relatively, a score by about e sqrt(D) scale: tens of bf16 bounds, but fewer than ten fp16 ones -
              required of bf16 gauss only"""
    assert case["group"] == "scale"
    if plant == "defscale":
        return case["scale"] != DC.scale_of("def", case["D"])
    if plant == "noscale":
        return case["scale"] != 1.0
    if plant == "qscaled":
        return dtype == "bf16" and case["sname"] == "p3" and case["kind"] == "gauss"
    raise KeyError(plant)


def exact_under_qscaled(case, dtype):
    return case["sname"] in ("one", "four") or (case["sname"] == "tiny" and dtype == "bf16")


def planted(plant, q, ks, vs, scale, dtype):
    """(out, lse) of the witness's arithmetic with one error planted"""
    if plant == "defscale":
        return W.witness(q, ks, vs, float(np.float32(q.shape[-1] ** -0.5)))
    if plant == "noscale":
        return W.planted("noscale", q, ks, vs, scale)
    if plant == "qscaled":
        return W.witness(C.to_elem(q * np.float32(scale), dtype), ks, vs, 1.0)
    raise KeyError(plant)


def test_case_list_covers_what_it_claims():
    cs = DC.CASES
    assert len({c["id"] for c in cs}) == len(cs) == 184
    assert all(c["B"] <= 2 and c["H"] in (2, 3) and len(DC.lengths(c)) <= 16 and sum(DC.lengths(c)) <= 400 for c in cs)
    f = np.float32
    for D in (64, 72, 88, 120, 128):
        assert [DC.scale_of(s, D) for s in DC.SCALE_NAMES] == [1.0, float(f(0.3)), float(f(f(1 / 3) * f(D ** -0.5))), 2.0 ** -20, 4.0]
        assert DC.scale_of("def", D) == float(f(D ** -0.5)) and DC.scale_of("sub", D) == 2.0 ** -149 == DC.SUBNORMAL
        assert all(float(f(DC.scale_of(s, D))) == DC.scale_of(s, D) > 0.0 for s in DC.SCALE_NAMES + ("def", "sub"))
    assert DC.DIMS == {"eq": (64, 128), "var": (64, 128), "hd": (72, 88, 120)}
    # every scale x entry point x D x two shapes x type, gaussian, Sq 33, B 2; peak, ramp at fp32(0.3) and the subnormal once each
    for ep in DC.ENTRIES:
        for dtype in TDT:
            for D in DC.DIMS[ep]:
                for sname in DC.SCALE_NAMES:
                    got = DC.of(ep, "scale", dtype, kind="gauss", D=D, sname=sname, Sq=33, B=2)
                    assert [DC.lengths(c) for c in got] == ([[65] * 3, [100] * 2] if ep == "eq" else [[65, 64, 63], [100, 37, 128, 5]]), (ep, D, sname)
            for kind in ("peak", "ramp"):
                assert len(DC.of(ep, "scale", dtype, kind=kind, sname="p3")) == 1
            sub, = DC.of(ep, "scale", dtype, sname="sub")
            assert sub["kind"] == "gauss" and sub["scale"] == 2.0 ** -149
        assert {c["sname"] for c in DC.of(ep, "scale")} == set(DC.SCALE_NAMES) | {"sub"}          # (never D ** -0.5 itself)
    # every flat kind x list x D x type for var and hd; the single key at every D at two scales
    for ep in ("var", "hd"):
        for dtype in TDT:
            for D in DC.DIMS[ep]:
                for kind in DC.FLAT_KINDS:
                    assert [c["sks"] for c in DC.of(ep, "kind", dtype, kind=kind, D=D)] == [[65, 64, 63], [100, 37, 128, 5], list(range(1, 17))]
            for D in DC.INT_DIMS[ep]:
                assert [c["sname"] for c in DC.of(ep, "int", dtype, D=D, sks=[1])] == ["def", "p3"]
            assert len(DC.of(ep, "int", dtype, sks=[1, 1, 1])) == 1
    assert DC.INT_DIMS["hd"] == (72, 80, 88, 96, 104, 112, 120) and not DC.of("eq", "kind") and not DC.of("eq", "int")
    # every Sq for every entry point, fp16, B 1, gaussian at the default scale; bf16 at the two whole-tile counts
    assert DC.SQS == (31, 32, 63, 64, 65, 127, 128, 255, 256, 257) and {ep for ep, _ in DC.SQ_DIMS} == set(DC.ENTRIES)
    for ep, D in DC.SQ_DIMS:
        got = DC.of(ep, "sq", "fp16", D=D)
        assert [c["Sq"] for c in got] == list(DC.SQS) and all(c["B"] == 1 and c["kind"] == "gauss" and c["sname"] == "def" for c in got)
        assert {tuple(DC.lengths(c)) for c in got} == ({(65, 65, 65)} if ep == "eq" else {(65, 64, 63)})
        assert [c["Sq"] for c in DC.of(ep, "sq", "bf16", D=D)] == [128, 256, 257]
    # the shapes that are not the ones named: stated, and nothing else moved
    assert [m[0] for m in DC.MOVED] == ["sq: eq on [65, 64, 63]"] and all(len(m) == 3 and m[2] for m in DC.MOVED)


def test_every_built_value_is_a_value_of_its_type_and_the_scale_is_the_cases():
    bases = {}
    for c in DC.CASES:
        for dtype in c["dtypes"]:
            q, ks, vs, scale = DC.build(c, dtype)
            lens = DC.lengths(c)
            assert q.shape == (c["B"], c["Sq"], c["H"], c["D"]) and [k.shape for k in ks] == [(c["B"], n, c["H"], c["D"]) for n in lens] == [v.shape for v in vs]
            assert scale == c["scale"] == DC.scale_of(c["sname"], c["D"])
            for x in [q] + ks + vs:
                assert x.dtype == np.float32 and np.array_equal(C.to_elem(x, dtype), x), c["id"]
                assert torch.equal(torch.from_numpy(x).to(TDT[dtype]).float(), torch.from_numpy(x)), c["id"]
            if c["kind"] == "zeroq":
                assert not q.any()
            if c["kind"] == "equal":
                assert (q == 0.5).all() and all((k == 0.25).all() for k in ks)
            if c["kind"] == "vmax":
                assert all((np.abs(v) == (65504.0 if dtype == "fp16" else 2.0 ** 100)).all() for v in vs)
            if c["kind"] == "int":
                assert all((x == np.round(x)).all() and np.abs(x).max() <= 3 for x in [q] + ks)
            if c["group"] == "sq":                                   # one q, one set of blocks for every Sq of an entry point and D
                key = (DC.sq_base(c)["id"], dtype)
                if key not in bases:
                    bases[key] = DC.build(DC.sq_base(c), dtype)
                bq, bks, bvs, _ = bases[key]
                assert np.array_equal(q, bq[:, :c["Sq"]]) and all(np.array_equal(a, b) for a, b in zip(ks + vs, bks + bvs))


def test_the_bounds_are_the_existing_ones_and_carry_the_scale():
    """no new witness, bound or constant; on equal lengths the two bounds are the same numbers at a scale that is no power of two; the
    lse bound of every gaussian scale case stays between 5e-6 and 1e-2 (8.8e-6 .. 7.2e-3): a wrong scale moves lse by tenths"""
    assert VW.witness is W.witness and VW.check is W.check and not [n for n in dir(DC) if n in ("U", "SLACK", "EPS", "SUB", "reference_and_bound", "check")]
    case = DC.of("eq", "scale", kind="gauss", D=64, sname="p3")[0]
    q, ks, vs, scale, ref = ref_of(case, "bf16")
    for a, b in zip(ref, VW.reference_and_bound(q, ks, vs, scale, "bf16")):
        assert np.array_equal(a, b)
    lo, hi = np.inf, 0.0
    for c in DC.of(group="scale", kind="gauss"):
        for dtype in c["dtypes"]:
            lb = ref_of(c, dtype)[4][3]
            lo, hi = min(lo, lb.min()), max(hi, lb.max())
    print(f"lse bounds of the gaussian scale cases: {lo:.2e} .. {hi:.2e}")
    assert 5e-6 <= lo and hi <= 1e-2
    # the subnormal scale: every score zero or subnormal, the weights uniform, lse = log K
    for ep in DC.ENTRIES:
        c, = DC.of(ep, "scale", sname="sub")
        q, ks, vs, scale, ref = ref_of(c, "fp16")
        s, _ = W.scores(q, ks, scale)
        assert np.abs(s).max() < 2.0 ** -126 and np.abs(ref[1] - np.log(sum(DC.lengths(c)))).max() < 1e-30


@pytest.mark.parametrize("dtype", list(TDT))
@pytest.mark.parametrize("plant", PLANTS)
def test_a_wrong_scale_exceeds_the_bound_tenfold(plant, dtype):
    """every scale case that can show the planted error (can_show: from the case alone) does, by 10 x the bound on out or lse; where it
    cannot because the arithmetic is exact there - the scale IS the planted one, or a power of two under `qscaled` - the plant returns the
    witness bit for bit: why 1.0 and 4.0 alone would not hold the scale product to its one fp32 rounding"""
    shown, exact, missed = {}, 0, []
    for c in DC.of(group="scale", dtype=dtype):
        q, ks, vs, scale, ref = ref_of(c, dtype)
        got = planted(plant, q, ks, vs, scale, dtype)
        fo, fl = W.excess(*got, ref)
        if can_show(plant, c, dtype):
            assert max(fo, fl) >= 10.0, f"{plant} on {c['id']} {dtype}: only {fo:.2f} / {fl:.2f} x the bound (out / lse)"
            shown[c["ep"], c["sname"]] = min(shown.get((c["ep"], c["sname"]), np.inf), max(fo, fl))
        elif plant != "qscaled" or exact_under_qscaled(c, dtype):
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (plant, c["id"], dtype)
            exact += 1
        else:
            missed.append((c["id"], round(max(fo, fl), 1)))          # qscaled where it is neither exact nor required: listed, not asserted
    print(plant, dtype, {k: f"{v:.3g}" for k, v in shown.items()}, "exact:", exact, "not required:", missed)
    if plant == "defscale":
        assert set(shown) == {(ep, s) for ep in DC.ENTRIES for s in DC.SCALE_NAMES + ("sub",)} and exact == 0
    elif plant == "noscale":
        assert set(shown) == {(ep, s) for ep in DC.ENTRIES for s in DC.SCALE_NAMES[1:] + ("sub",)} and exact == sum(len(DC.DIMS[ep]) * 2 for ep in DC.ENTRIES)
    else:
        assert set(shown) == ({(ep, "p3") for ep in DC.ENTRIES} if dtype == "bf16" else set())
        n = sum(len(DC.DIMS[ep]) * 2 for ep in DC.ENTRIES)
        assert exact == (3 * n if dtype == "bf16" else 2 * n)


@pytest.mark.parametrize("dtype", list(TDT))
def test_one_key_gained_in_a_tail_tile_shows_in_every_flat_case(dtype):
    """zeroq / equal on unequal lengths: every key weighs the same, so the key COUNT is all that lse holds.  One zero row of a block's
    tail tile scored as a real key (_attn_var_f64._masked with eff = own + 1, in the first block that has a tail) moves lse by about
    1 / K: more than ten lse bounds in every such case."""
    n = 0
    for c in DC.of(group="kind", dtype=dtype):
        if c["kind"] not in ("zeroq", "equal"):
            continue
        q, ks, vs, scale, ref = ref_of(c, dtype)
        i = next(i for i, k in enumerate(c["sks"]) if k % 64)
        k1, v1 = VW._masked(ks[i], vs[i], c["sks"][i], c["sks"][i] + 1)
        assert k1.shape[1] == c["sks"][i] + 1
        _, fl = W.excess(*W.witness(q, ks[:i] + [k1] + ks[i + 1:], vs[:i] + [v1] + vs[i + 1:], scale), ref)
        assert fl >= 10.0, f"{c['id']} {dtype}: a gained key moves lse by {fl:.2f} bounds only"
        n += 1
    assert n == 2 * 3 * (len(DC.DIMS["var"]) + len(DC.DIMS["hd"]))


def test_zero_queries_and_single_keys_are_what_the_header_says():
    """zeroq: the witness is the same at every scale (0 * scale = 0).  int, one key: out is v and lse the exact a * scale, whose fp32
    rounding is the ONE rounding the launch makes - |a| <= 9 D < 2^24, so a itself is an fp32 value"""
    c = DC.of("var", "kind", kind="zeroq", D=64, sks=[65, 64, 63])[0]
    q, ks, vs, scale, ref = ref_of(c, "fp16")
    for sname in DC.SCALE_NAMES:
        o, l = W.witness(q, ks, vs, DC.scale_of(sname, 64))
        assert np.array_equal(o, ref[0]) and np.array_equal(l, ref[1])
    for c in DC.of(group="int", sks=[1]):
        q, ks, vs, scale, ref = ref_of(c, "bf16")
        a = (q.astype(np.float64) * ks[0].astype(np.float64)).sum(-1)
        assert np.abs(a).max() < 2 ** 24 and np.array_equal(a, np.round(a))
        assert np.array_equal(ref[0], np.broadcast_to(vs[0].astype(np.float64), ref[0].shape)) and np.array_equal(ref[1], a * scale)


@pytest.mark.parametrize("dtype", list(TDT))
def test_the_eager_definition_honours_the_callers_scale(dtype, monkeypatch):
    """attention_blocks(q, ks, vs, scale) on CPU tensors - the definition a launch is refused to - within the bound at fp32(0.3) for
    every entry point's shape, and NOT within it of the default-scale witness"""
    from compactfusion_amd.compact import attention as A
    monkeypatch.setattr(A, "_attn_fwd_native", lambda *a, **k: pytest.fail("CPU tensors reached the native launch"))
    monkeypatch.setattr(A, "_attn_fwd_native_var", lambda *a, **k: pytest.fail("CPU tensors reached the native launch"))
    for ep in DC.ENTRIES:
        c = DC.of(ep, "scale", kind="gauss", sname="p3")[0]
        q, ks, vs, scale, ref = ref_of(c, dtype)
        t = lambda x: torch.from_numpy(x).to(TDT[dtype])       # noqa: E731
        out, lse = A.attention_blocks(t(q), [t(k) for k in ks], [t(v) for v in vs], scale)
        W.check(out.float().numpy(), lse.transpose(1, 2).numpy(), ref, f"attention_blocks, eager, {c['id']}")
        out, lse = A.attention_blocks(t(q), [t(k) for k in ks], [t(v) for v in vs])
        assert max(W.excess(out.float().numpy(), lse.transpose(1, 2).numpy(), ref)) >= 10.0
