"""The value domain of the int8, int4 and top-k codecs (tests/_value_cases.py) on the CPU: the numpy oracle against the float64 definition
(tests/_f64_check.py) on every finite case at every shape tests/test_gpu_value_domain.py runs, the numpy and the C oracle bit for bit
(int4's `min` half under the signed-zero rule of tests/_zero_min.py and nothing more), the proof - counted from the data - that every case
holds what its `why` says, and planted errors that the check must reject.  CPU only."""
import numpy as np
import pytest

import _f64_check as F
import _nonfinite as NF
import _value_cases as V
import _zero_min as Z
from oracle import c_oracle as CO
from oracle import ref_np as R

F16, F64 = np.float16, np.float64
CODECS = [("int8", 0), ("int4", 0)] + [("topk", m) for m in V.TOPK_M]


def oracle(codec, param, x, base):
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        pkt, nb = R.residual_compress(codec, x, base, param) if base is not None else R.compress(codec, x, None, param)
    return np.asarray(pkt).view(np.uint16), R.bits(nb)


def _all():
    out = []
    for codec, param in CODECS:
        for N, C in V.shapes_for(codec):
            for case in V.cases_for(codec, N, C, param):
                out.append(pytest.param(codec, param, case, N, C, id=f"{codec}{param or ''}-{case}-{N}x{C}"))
    return out


@pytest.mark.parametrize("codec,param,case,N,C", _all())
def test_oracles_meet_the_definition_and_each_other(codec, param, case, N, C):
    """every draw the GPU module uses (at least two: the gated call's two items), with a base over two rounds of error feedback - the second
    round's residual is the first round's quantisation error - and with base None"""
    planted = V.signed_zero_channels(case, N, C)
    for nobase in (False, True):
        for rep in range(max(2, V.reps(case, N, C))):
            x, base = V.build(case, codec, N, C, rep=rep, param=param, nobase=nobase)
            assert np.isfinite(x).all() and (base is None or np.isfinite(base).all())
            assert np.isfinite(V.delta(x, base)).all(), "the case leaves the domain |x - base| < 65504"
            for t in range(1 if nobase else 2):
                pkt, nb = oracle(codec, param, x, base)
                if case in V.FINITE:
                    F.check(codec, param, x, base, pkt, nb)
                else:
                    assert t or not np.isfinite(pkt.view(F16)[-2 * C:-C]).all(), "range-overflow: every scale is finite"
                pkt_c, nb_c = CO.compress(codec, x, base, N, C, param)
                allowed = Z.same_packet(codec, pkt_c, pkt, x, base, "C oracle packet")
                assert allowed <= planted, allowed
                NF.same_bits(nb_c, nb, "C oracle state")
                NF.same_bits(CO.decompress(codec, pkt, base, N, C, param), nb, "C oracle reconstruction")
                base = nb.view(F16).reshape(N, C)


# ---- every case holds what its `why` says (counted from d, not from the generator's intent) ---------------------------------------------
def _d(case, codec, N, C, **kw):
    return V.delta(*V.build(case, codec, N, C, **kw))


@pytest.mark.parametrize("N,C", V.MINMAX_SHAPES)
def test_extremes_are_placed_on_every_row_class(N, C):
    rows = set()
    for rep in range(V.reps("extremes-placed", N, C)):
        d = _d("extremes-placed", "int8", N, C, rep=rep).astype(F64)
        mn, mx = d.min(axis=0), d.max(axis=0)
        if N > 1:
            assert ((d == mn).sum(axis=0) == 1).all() and ((d == mx).sum(axis=0) == 1).all(), "an extreme occurs twice: the rest is not strictly inside"
        amin, amax = d.argmin(axis=0), d.argmax(axis=0)
        rows |= set(amin.tolist()) | set(amax.tolist())
        assert {amin[C - 1], amax[C - 1]} == {0, N - 1}                          # channel C - 1: the last active lane of the last column block
    want = set(V.extreme_rows(N))
    assert want <= rows, sorted(want - rows)
    assert {0, N - 1} <= rows and {r % 8 for r in rows} >= set(range(min(8, N)))
    for b in range(32, N, 32):                                                  # both sides of every 32-row (and with them 64-row) boundary
        assert b - 1 in rows and b in rows, b


def test_constant_and_one_unit_channels():
    for N, C in V.MINMAX_SHAPES:
        d = _d("constant-channels", "int4" if N % 2 == 0 else "int8", N, C)
        u, d64 = d.view(np.uint16), d.astype(F64)
        rng = d64.max(axis=0) - d64.min(axis=0)
        assert (u[:, 0] == 0).all() and (d64[:, 1] == 0.5).all() and (rng[8:16] == 0).all()
        if N > 1:
            assert (rng[[2, 3, 4]] == 2.0 ** -24).all()
            pkt, _ = oracle("int8", 0, d, None)
            assert (pkt.view(F16)[-2 * C:-C][[2, 3, 4]] == 0).all(), "a range of one unit must round to scale 0"
            assert (rng > 2.0 ** -10).sum() >= (C - 512 - 8 if C > 512 else C - 20), "the ordinary channels are missing"
        if C > 512:
            assert (rng[:512] == 0).sum() >= 509 and len(set(d64[0, :512].tolist())) >= 9
    x, base = V.build("constant-channels", "int8", 66, 144)
    assert (x[:, 1].astype(F64) - base[:, 1].astype(F64) == 0.5).all() and len(set(base[:, 1].tolist())) > 8, "x = base + 0.5 exactly, over a varying base"


def test_signed_zero_extremes_in_tiles_and_waves():
    seen = set()
    for N, C in V.MINMAX_SHAPES:
        if N < 2:
            continue
        d = _d("signed-zero-extremes", "int8", N, C)
        u, d64 = d.view(np.uint16), d.astype(F64)
        both = (u == 0).any(axis=0) & (u == 0x8000).any(axis=0)
        zmin, zmax = both & (d64.min(axis=0) == 0), both & (d64.max(axis=0) == 0)
        assert set(np.flatnonzero(zmin).tolist()) == V.signed_zero_channels("signed-zero-extremes", N, C)
        assert (zmin & zmax).any() and (N == 2 or ((zmin & ~zmax).any() and (zmax & ~zmin).any()))
        for c in np.flatnonzero(zmin ^ zmax):
            neg, pos = np.flatnonzero(u[:, c] == 0x8000), np.flatnonzero(u[:, c] == 0)
            assert neg.size == 1 and pos.size == 1
            a, b = int(neg[0]), int(pos[0])
            kind = "min" if zmin[c] else "max"
            if a // 32 != b // 32:
                seen.add((kind, "tiles", a < b))
            elif a % 8 != b % 8:
                seen.add((kind, "waves", a < b))
        if N > 64:
            assert {(k, "tiles", o) for k in ("min", "max") for o in (True, False)} <= seen, (N, C, seen)
    assert {(k, w, o) for k in ("min", "max") for w in ("tiles", "waves") for o in (True, False)} <= seen, seen


def test_offset_saturates_the_zero_point_both_ways_and_codes_clamp():
    for N, C in V.MINMAX_SHAPES:
        if N < 2:
            continue
        x, base = V.build("offset", "int8", N, C)
        d = V.delta(x, base).astype(F64)
        assert ((d >= 100) & (d <= 101) | (d >= -2000) & (d <= -1990)).all()
        pkt, _ = oracle("int8", 0, x, base)
        zp, q = pkt[-C:].view(np.int16), pkt[:N * C // 2].view(np.int8)
        assert (zp == -128).sum() == C // 2 and (zp == 127).sum() == C // 2, (N, C)
        assert (q == 127).any() and (q == -128).any()


def test_tiny_wide_and_overflow_ranges():
    for N, C in V.MINMAX_SHAPES:
        d = _d("tiny", "int8", N, C).astype(F64) * 2.0 ** 24
        assert (d == np.rint(d)).all() and np.abs(d[:, 0::2]).max() <= 40 and np.abs(d).max() <= 320
        if N < 2:
            continue
        for codec, lv in (("int8", 255), ("int4", 15)):
            if V.legal(codec, N, C):
                pkt, _ = oracle(codec, 0, *V.build("tiny", codec, N, C))
                s = pkt.view(F16)[-2 * C:-C].astype(F64)
                assert (s < 2.0 ** -14).all() and (s > 0).any() and (lv == 15 or (s == 0).any())
        d = _d("wide", "int8", N, C).astype(F64)
        r = d.max(axis=0) - d.min(axis=0)
        assert (r > 32768).all() and (r < 65504).all() and (r.astype(F16).astype(F64) != r).any(), "fp16(max - min) never rounds"
        d = _d("range-overflow", "int8", N, C).astype(F64)
        assert np.abs(d).max() == 60000 and ((d.max(axis=0) - d.min(axis=0)) > 65520).sum() >= 3
    x, base = V.build("tiny", "int4", 66, 144)
    assert (base != 0).mean() > 0.9, "tiny: the base is not ordinary"


def test_rint_ties_are_ties():
    for codec, lo, hi in (("int4", 0.0, 15.0), ("int8", -100.0, 155.0)):
        for N, C in V.shapes_for(codec):
            x, base = V.build("rint-ties", codec, N, C)
            d = V.delta(x, base).astype(F64)
            pkt, _ = oracle(codec, 0, x, base)
            s = pkt.view(F16)[-2 * C:-C].astype(F64)
            if N < 2:
                continue
            assert (s == 1.0).all() and (d.min(axis=0) == lo).all() and (d.max(axis=0) == hi).all()
            t = d - lo if codec == "int4" else d + pkt[-C:].view(np.int16).astype(F64)
            halves = int((t - np.floor(t) == 0.5).sum())
            assert halves == (N - 2) * C, (codec, N, C, halves)
            if N > 8:
                k = np.floor(t[t - np.floor(t) == 0.5])
                assert (k % 2 == 0).any() and (k % 2 == 1).any()


def test_near_tie_quotients_need_the_correctly_rounded_division():
    """the planted quotients exist in the data (counted from d and the oracle's packet), and an fp32 quotient formed as a * rcp(s) without
    hdiv_r's correcting step - rcp(s) the correctly rounded reciprocal or a unit in the last place beside it, as v_rcp_f32 may return -
    sends some of them to the neighbouring code: the case decides whether the step is there"""
    N, C = 66, 144
    seen, moved = 0, {0: 0, 1: 0, -1: 0}
    for rep in range(V.reps("near-tie-quotients", N, C)):
        x, base = V.build("near-tie-quotients", "int8", N, C, rep=rep)
        d = V.delta(x, base)
        pkt, _ = oracle("int8", 0, x, base)
        s, zp = pkt.view(F16)[-2 * C:-C], pkt[-C:].view(np.int16)
        q = pkt[:N * C // 2].view(np.int8).reshape(N, C)
        assert (zp == -128).all() and (d.astype(F64).min(axis=0) == 0).all()
        t = d.astype(F64) / s.astype(F64)[None, :]
        lo = t.astype(F16)
        other = np.where(lo.astype(F64) < t, np.nextafter(lo, F16(np.inf)), np.nextafter(lo, F16(0))).astype(F64)
        mid = (lo.astype(F64) + other) / 2
        with np.errstate(invalid="ignore", divide="ignore"):
            near = (np.abs(t - mid) < mid * 2.0 ** -22) & (np.rint(lo.astype(F64)) != np.rint(other))
        seen += int(near.sum())
        for k in moved:
            rb = (np.float32(1.0) / s.astype(np.float32))
            for _ in range(abs(k)):
                rb = np.nextafter(rb, np.float32(np.inf if k > 0 else 0))
            t32 = d.astype(np.float32) * rb[None, :]
            code = np.clip(np.rint((t32.astype(F16) + zp.astype(F16)[None, :]).astype(F16)), -128, 127)
            moved[k] += int((code != q).sum())
    assert seen >= 200, seen
    assert max(moved.values()) > 0, moved


def test_topk_cases_hold_what_they_claim():
    for N, C in V.TOPK_SHAPES:
        straddle = (1024 % C != 0) or C > 1024
        for m in V.TOPK_M:
            a = np.abs(_d("ties", "topk", N, C, param=m).astype(F64)).reshape(-1, m)
            assert set(np.unique(_d("ties", "topk", N, C, param=m).astype(F64)).tolist()) == {-0.75, -0.5, -0.25, 0.0, 0.25, 0.5, 0.75}
            if m > 2:
                assert ((a == a.max(axis=1, keepdims=True)).sum(axis=1) > 1).mean() > 0.3
            d = _d("kept-index-sweep", "topk", N, C, param=m).astype(F64).reshape(-1, m)
            a = np.abs(d)
            assert ((a == a.max(axis=1, keepdims=True)).sum(axis=1) == 1).all(), "the maximum is not single"
            am = a.argmax(axis=1)
            assert set(am.tolist()) == set(range(m))
            if straddle and m > 1 and C % m:
                first = (np.arange(am.size) * m) // C
                last = (np.arange(am.size) * m + m - 1) // C
                assert set(am[first != last].tolist()) == set(range(m)), "half-blocks that straddle rows do not see every index"
            x, base = V.build("zero-half-blocks", "topk", N, C, param=m)
            u = V.delta(x, base).view(np.uint16).reshape(-1, m)
            z = ((u & 0x7FFF) == 0).all(axis=1)
            assert z.sum() >= u.shape[0] // 2 and (u[z, 0] == 0x8000).all()
            pkt, nb = oracle("topk", m, x, base)
            kept0 = pkt[:N * C // m][z]
            assert (kept0 == 0x8000).all(), "the kept value of a zero half-block is d[0] = -0 bit for bit"
            if m > 1:
                under = (base.view(np.uint16).reshape(-1, m)[z][:, 1:] == 0x8000)
                assert under.sum() > 0 and (nb.reshape(-1, m)[z][:, 1:][under] == 0).all()      # (-0) + (+0) = +0
            d = _d("subnormal-and-max", "topk", N, C, param=m).astype(F64).reshape(-1, m)
            a = np.abs(d)
            assert ((a < 2.0 ** -14).all(axis=1) & (a > 0).any(axis=1)).sum() > 10 and (a == 65504).any(axis=1).sum() > 10
            if m > 1:
                assert ((a == 65504).sum(axis=1) == 2).any()
        d = _d("cross-lane-ties", "topk", N, C, param=16).astype(F64).reshape(-1, 16)
        a = np.abs(d)
        top = a == a.max(axis=1, keepdims=True)
        assert (top[:, :8].any(axis=1) & top[:, 8:].any(axis=1)).all(), "a half-block without a cross-lane tie"
        seen = set()
        for h in range(d.shape[0]):
            i = np.flatnonzero(top[h])
            lo_i, hi_i = int(i[i < 8][0]), int(i[i >= 8][0])
            seen.add((lo_i, hi_i, bool(d[h, lo_i] > 0), bool(d[h, hi_i] > 0)))
        want = {(a_, b_, sa, sb) for a_, b_ in ((3, 11), (7, 8), (0, 15)) for sa in (True, False) for sb in (True, False)}
        assert want <= seen, want - seen
        assert (top.sum(axis=1) == 3).any()                                      # a tie inside the lower lane AND across lanes
        if straddle and C % 16:
            hb0 = np.arange(d.shape[0]) * 16
            st = (hb0 // C) != ((hb0 + 15) // C)
            assert st.any() and ((hb0[st] + 8) % C == 0).any(), "no straddling half-block whose upper lane is the later row"


# ---- the check rejects planted errors -------------------------------------------------------------------------------------------------
def _int4_codes(pkt, N, C):
    return pkt[:N * C // 4].view(np.uint8).reshape(N // 2, C)


def test_rejects_a_tie_rounded_away_from_even():
    N, C = 66, 144
    x, base = V.build("rint-ties", "int4", N, C)
    pkt, nb = oracle("int4", 0, x, base)
    F.check("int4", 0, x, base, pkt, nb)
    d = V.delta(x, base).astype(F64)
    r, c = [(r, c) for r in range(0, N, 2) for c in range(C) if d[r, c] % 2 == 0.5][0]          # k + 1/2 with k even: the code is k
    bad = pkt.copy()
    q = _int4_codes(bad, N, C)
    assert (q[r // 2, c] & 15) == int(d[r, c] - 0.5)
    q[r // 2, c] += 1
    with pytest.raises(AssertionError, match="exact quotients: 1/"):
        F.check("int4", 0, x, base, bad, None)
    x, base = V.build("rint-ties", "int8", N, C)
    pkt, nb = oracle("int8", 0, x, base)
    F.check("int8", 0, x, base, pkt, nb)
    t = V.delta(x, base).astype(F64) - 28.0
    away = np.where(t - np.floor(t) == 0.5, np.floor(t) + (t > 0), np.rint(t))                   # round half away from zero
    bad = pkt.copy()
    bad[:N * C // 2].view(np.int8)[:] = np.clip(away, -128, 127).astype(np.int8).reshape(-1)
    with pytest.raises(AssertionError, match="exact quotients"):
        F.check("int8", 0, x, base, bad, None)


def test_rejects_a_topk_index_moved_to_the_second_maximum():
    N, C, m = 128, 72, 16
    for case in ("ties", "cross-lane-ties"):
        x, base = V.build(case, "topk", N, C, param=m)
        pkt, nb = oracle("topk", m, x, base)
        F.check("topk", m, x, base, pkt, nb)
        d = V.delta(x, base).reshape(-1, m)
        a = np.abs(d.astype(F64))
        h = int(np.flatnonzero((a == a.max(axis=1, keepdims=True)).sum(axis=1) >= 2)[1])
        second = int(np.flatnonzero(a[h] == a[h].max())[1])
        bad = pkt.copy()
        bad[h] = d.view(np.uint16)[h, second]
        idx = bad[N * C // m:].view(np.uint8)
        idx[h // 2] = (idx[h // 2] & 0xF0) | second if h % 2 else (idx[h // 2] & 0x0F) | (second << 4)
        with pytest.raises(AssertionError, match="indices: 1/"):
            F.check("topk", m, x, base, bad, None)


@pytest.mark.parametrize("codec", ["int8", "int4"])
def test_rejects_a_scale_computed_without_the_last_row(codec):
    N, C = 66, 144
    x, base = V.build("extremes-placed", codec, N, C)
    pkt, nb = oracle(codec, 0, x, base)
    F.check(codec, 0, x, base, pkt, nb)
    short, _ = oracle(codec, 0, x[:N - 2], base[:N - 2])
    assert (short[-2 * C:-C] != pkt[-2 * C:-C]).any()
    bad = pkt.copy()
    bad[-2 * C:-C] = short[-2 * C:-C]
    with pytest.raises(AssertionError, match="scale"):
        F.check(codec, 0, x, base, bad, None)


def test_rejects_a_zero_point_left_unclamped():
    N, C = 66, 144
    x, base = V.build("offset", "int8", N, C)
    pkt, nb = oracle("int8", 0, x, base)
    F.check("int8", 0, x, base, pkt, nb)
    d = V.delta(x, base).astype(F64)
    s = pkt.view(F16)[-2 * C:-C].astype(F64)
    for c in (0, 1):
        bad = pkt.copy()
        bad[-C:].view(np.int16)[c] = int(np.clip(-128 - np.rint(d[:, c].min() / s[c]), -32768, 32767))      # (as far as the int16 holds it)
        with pytest.raises(AssertionError, match="zero point"):
            F.check("int8", 0, x, base, bad, None)


@pytest.mark.parametrize("codec", ["int8", "int4"])
def test_the_clamp_term_passes_tiny_and_still_rejects_errors(codec):
    """subnormal scales: the oracle passes (it did not for int4 before the clamp term), and a code one off, a scale two units off and a
    reconstruction one code short of d still fail"""
    N, C = 66, 144
    x, base = V.build("tiny", codec, N, C, nobase=True)
    pkt, nb = oracle(codec, 0, x, None)
    F.check(codec, 0, x, None, pkt, nb)
    d = x.astype(F64)
    c = 7
    r = int(d[:, c].argmax())
    bad = pkt.copy()
    if codec == "int4":
        q = _int4_codes(bad, N, C)
        q[r // 2, c] -= 1 << (4 * (r % 2))
    else:
        bad[:N * C // 2].view(np.int8).reshape(N, C)[r, c] -= 1
    with pytest.raises(AssertionError, match="codes"):
        F.check(codec, 0, x, None, bad, None)
    bad = pkt.copy()
    bad[-2 * C + c] += 2
    with pytest.raises(AssertionError, match="scale"):
        F.check(codec, 0, x, None, bad, None)
    bad = nb.copy()
    bad.reshape(N, C)[r, c] -= 1                  # the state one unit of 2^-24 off
    with pytest.raises(AssertionError, match="state elements"):
        F.check(codec, 0, x, None, pkt, bad)
    # the term itself: 0 on a normal scale, and on a subnormal one no more than the (levels - 1) / 2 units the scale's rounding can lose
    L = 255 if codec == "int8" else 15
    s = pkt.view(F16)[-2 * C:-C].astype(F64)
    term = F._clamp_term(s, d.min(axis=0), d.max(axis=0), L + 1)
    assert (term <= L / 2 * 2.0 ** -24 + 1e-12).all() and term.max() > 0
    assert (F._clamp_term(np.full(C, 2.0 ** -14), d.min(axis=0), d.max(axis=0), L + 1) == 0).all()
