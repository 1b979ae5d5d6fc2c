"""The float64 witness of the low-rank receiver (tests/_lr_f64_check.py) and its cases (tests/_lr_cases.py), on the CPU:

  * the witness ACCEPTS the fp32-matmul decode of tests/_oracle_backend.py on every case, LOW_RANK and LOW_RANK_Q;
  * it REJECTS planted errors: a pinned element one fp16 ulp off, two rows swapped, V indexed transposed, the ragged last row left
    stale, a k-lane dropped, a LOW_RANK_Q packet with its nibbles swapped;
  * every case holds what its `why` says;
  * the condition under which the interval test means something: on every `random` draw tests/test_gpu_lr_receiver.py decodes the
    witness ALONE pins at least 80 % of the elements, and 100 % on `integers` and `one-hot` (docs/DESIGN_DETAIL.md has the table)."""
import numpy as np
import pytest
import torch

import _lr_cases as LC
import _lr_f64_check as W
import _oracle_backend as OB

F16, F64 = np.float16, np.float64
SHAPES = [(False, 37, 1032, 18), (False, 5, 24, 2), (False, 33, 520, 32), (True, 34, 520, 24), (True, 6, 8, 8), (True, 70, 1032, 32)]


def t16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16).copy()).view(torch.float16)


def n16(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def decode(quant, pkt, base, N, C, r):
    """out bits of the stand-in backend: fp16(fp32 matmul), then the fp16 add"""
    recv = OB._lr_decode(quant, t16(pkt), N, C, r)
    out = recv if base is None else t16(base).view(N, C) + recv
    return n16(out).reshape(N, C)


def factors(quant, pkt, U, V, N, C, r):
    return W.split_q(pkt, N, C, r) if quant else (U, V)


@pytest.mark.parametrize("name", LC.NAMES)
@pytest.mark.parametrize("quant,N,C,r", SHAPES)
def test_witness_accepts_the_fp32_matmul_decode(quant, N, C, r, name):
    U, V, base = LC.build(name, N, C, r, 0, quant)
    pkt = LC.packet(quant, U, V)
    for b in (base, None):
        out = decode(quant, pkt, b, N, C, r)
        share = W.check_q(pkt, N, C, r, b, out, name) if quant else W.check(U, V, b, out, name)
        if name in LC.EXACT:
            assert share == 1.0, (name, share)


def _rejects(U, V, base, out, what):
    with pytest.raises(AssertionError):
        W.check(U, V, base, out, what)


@pytest.mark.parametrize("withbase", [True, False], ids=["base", "nobase"])
def test_witness_rejects_planted_errors(withbase):
    N, C, r = 37, 1032, 18
    U, V, base = LC.build("random", N, C, r)
    b = base if withbase else None
    good = decode(False, LC.plain_packet(U, V), b, N, C, r)
    W.check(U, V, b, good, "good")
    lo, hi = W.bounds(U, V, b)
    pinned = np.argwhere((lo.astype(F64) == hi.astype(F64)) & (lo != 0))
    for n, c in (pinned[0], pinned[len(pinned) // 2], pinned[-1]):               # one pinned element, one fp16 ulp either way
        for step in (1, -1):
            bad = good.copy()
            bad[n, c] = np.uint16(int(bad[n, c]) + step)
            _rejects(U, V, b, bad, "one ulp")
    bad = good.copy()
    bad[[3, 4]] = bad[[4, 3]]
    _rejects(U, V, b, bad, "rows swapped")
    bad = good.copy()
    bad[N - 1] = 0x7E00 if b is None else np.ascontiguousarray(b).view(np.uint16)[N - 1]      # what an in-place call would find there
    _rejects(U, V, b, bad, "ragged last row left stale")
    Vt = np.ascontiguousarray(V.reshape(C, r).T)                                  # the (r, C) block read as (C, r)
    _rejects(U, V, b, decode(False, LC.plain_packet(U, Vt), b, N, C, r), "V transposed")
    for k in (r - 1, 0, 8):
        Ud = U.copy()
        Ud[:, k] = 0
        _rejects(U, V, b, decode(False, LC.plain_packet(Ud, V), b, N, C, r), f"k-lane {k} dropped")
    # on one-hot a dropped or shifted k-lane is a wrong VALUE on whole rows
    U1, V1, b1 = LC.build("one-hot", N, C, r)
    bb = b1 if withbase else None
    W.check(U1, V1, bb, decode(False, LC.plain_packet(U1, V1), bb, N, C, r), "one-hot")
    _rejects(U1, V1, bb, decode(False, LC.plain_packet(np.roll(U1, 1, axis=1), V1), bb, N, C, r), "k-lanes shifted")
    _rejects(U1, V1, bb, decode(False, LC.plain_packet(U1[:, :r - 2], V1[:r - 2]), bb, N, C, r - 2), "k-lanes r - 2, r - 1 dropped")


@pytest.mark.parametrize("name", ["random", "integers"])
def test_witness_rejects_a_q_packet_with_swapped_nibbles(name):
    N, C, r = 34, 520, 24
    U, V, base = LC.build(name, N, C, r, 0, True)
    pkt = LC.q_packet(U, V)
    W.check_q(pkt, N, C, r, base, decode(True, pkt.view(np.uint16), base, N, C, r), "good")
    for lo_, hi_ in ((0, N * r // 2), (N * r // 2 + 4 * r, N * r // 2 + 4 * r + C * r // 2)):      # the codes of U, of V^T
        bad = pkt.copy()
        bad[lo_:hi_] = (bad[lo_:hi_] >> 4) | ((bad[lo_:hi_] & 0x0F) << 4)
        with pytest.raises(AssertionError):
            W.check_q(pkt, N, C, r, base, decode(True, bad.view(np.uint16), base, N, C, r), "nibbles swapped")


def test_q_split_is_the_int4_contract():
    """the witness's own dequantiser (float64, two fp16 roundings) against oracle/ref_np.py on packets of the pinned oracle"""
    from oracle import ref_np as R
    for name in LC.NAMES:
        N, C, r = 70, 24, 8
        U, V, _ = LC.build(name, N, C, r, 0, True)
        pkt = LC.q_packet(U, V)
        Uq, Vq = W.split_q(pkt, N, C, r)
        nu = N * r // 2 + 4 * r
        assert np.array_equal(Uq.view(np.uint16), R.bits(R.decompress("int4", pkt[:nu].view(np.uint16), N, r)))
        assert np.array_equal(Vq.T.copy().view(np.uint16), R.bits(R.decompress("int4", pkt[nu:].copy().view(np.uint16), C, r)))


@pytest.mark.parametrize("quant,N,C,r", SHAPES + [(False, 1, 8, 32), (True, 2, 8, 32), (False, 129, 11784, 32)])
def test_cases_hold_what_they_say(quant, N, C, r):
    for name in LC.NAMES:
        U, V, base = LC.build(name, N, C, r, 0, quant)
        U2, V2, base2 = LC.build(name, N, C, r, 0, quant)
        assert np.array_equal(U.view(np.uint16), U2.view(np.uint16)) and np.array_equal(V.view(np.uint16), V2.view(np.uint16)) \
            and np.array_equal(base.view(np.uint16), base2.view(np.uint16)), "build is deterministic"
        Uf, Vf = factors(quant, LC.q_packet(U, V), U, V, N, C, r) if quant else (U, V)
        u, v, b = Uf.astype(F64), Vf.astype(F64), base.astype(F64)
        p = u @ v
        lo, hi = W.bounds(Uf, Vf, base)
        assert np.isfinite(lo).all() and np.isfinite(hi).all(), name
        if name == "integers":
            assert (u == np.rint(u)).all() and (v == np.rint(v)).all() and (b == np.rint(b)).all() and np.abs(u).max() <= 8 and np.abs(v).max() <= 8
            assert np.abs(u).max() == 8 and (np.abs(u) @ np.abs(v)).max() <= 2048          # every partial sum is an integer fp32 holds
            assert np.array_equal(lo.view(np.uint16), hi.view(np.uint16))
            assert np.array_equal(lo.view(np.uint16), (b + p.astype(F16).astype(F64)).astype(F16).view(np.uint16))
            if quant:                                                                      # the quantiser reproduced the factors exactly
                assert np.array_equal(Uf, U) and np.array_equal(Vf, V)
        if name == "one-hot":
            n = np.arange(N)
            hot = np.zeros((N, r), bool)
            hot[n, n % r] = True
            assert ((u != 0) == hot).all()
            assert np.array_equal(p, u[n, n % r][:, None] * v[n % r])                      # one term: exact in any order
            assert np.array_equal(lo.view(np.uint16), hi.view(np.uint16))
            if quant:
                assert np.array_equal(Uf, U) and np.array_equal(Vf, V)
                assert (v[:-1] != v[1:]).mean() > 0.9
            else:
                assert all(len(np.unique(V[:, c].view(np.uint16))) == r for c in range(0, C, max(1, C // 64)))
                assert all(len(np.unique(V[k, :16381 // r].view(np.uint16))) == min(C, 16381 // r) for k in range(r))
                if C == r:
                    assert not np.array_equal(V, V.T)
        if name == "large":
            t = LC.large_target(quant)
            assert np.abs(p).max() <= 1.15 * t and np.abs(b + p).max() < 65504 - 1000
            if not quant:
                assert abs(p[0, 0] - t) < 0.01 * t and abs(p[0, C - 1] + t) < 0.01 * t
            else:
                assert np.abs(p).max() > 0.8 * t
        if name == "zero-rows" and not quant:
            z = LC.zero_rows(N)
            assert z and (U[z] == 0).all() and (np.abs(u).sum(axis=1)[[i for i in range(N) if i not in z]] > 0).all()
            bz = base.view(np.uint16)[z]
            assert set(np.unique(bz).tolist()) == {0x0000, 0x8000}
            assert (lo[z] == 0).all() and (hi[z] == 0).all()
        if name == "subnormal-factors" and not quant:
            su, sv = W._subnormal(U), W._subnormal(V)
            assert su.mean() > 0.2 and sv.mean() > 0.2 and (~su).mean() > 0.5
            assert (U.astype(F64)[su] / LC.ULP0 == np.rint(U.astype(F64)[su] / LC.ULP0)).all()


def test_walk_shapes_take_the_row_counts_they_are_listed_for():
    for quant, N, C, rows in LC.WALK:
        assert LC.rows_per_wg(N, C, LC.WALK_BATCH) == rows, (N, C)
        assert not quant or N % 2 == 0
    # ... and nothing else among the GPU shapes leaves 32 rows, the product's (4096, 1152) x 14 does
    assert all(LC.rows_per_wg(N, C, 8) == 32 for N in LC.NS + LC.NS_Q for C in LC.CS)
    assert LC.rows_per_wg(544, 3072, 3) == 32 and LC.rows_per_wg(4096, 1152, 14) == 128


def _share(cache, quant, N, C, r, rep, withbase):
    key = (quant, N, C, r, rep)
    if key not in cache:
        U, V, base = LC.build("random", N, C, r, rep, quant)
        if quant:
            U, V = W.split_q(LC.q_packet(U, V), N, C, r)
        cache.clear()                     # (a draw is asked for with and without its base back to back)
        cache[key] = (U, V, base)
    U, V, base = cache[key]
    return W.pinned_share(U, V, base if withbase else None)


def test_the_witness_pins_most_of_every_random_draw_the_gpu_tests_use():
    """Condition, not measurement: an element is pinned where fp16(p - e) == fp16(p + e) and the add of the base keeps it so - a property
    of the draw and the derived bound alone."""
    cache = {}
    draws = LC.gpu_random_draws()
    assert len(draws) > 400
    for quant, N, C, r, rep, withbase in draws:
        s = _share(cache, quant, N, C, r, rep, withbase)
        assert s >= LC.PIN_MIN, (quant, N, C, r, rep, withbase, s)
    # the shapes' draws are the first that meet the condition: rep 0 with a base everywhere, and without a base all but a few tiny ones
    late = [d for d in draws if d[4] != (0 if d[5] else 1) and d[1:3] not in [s[1:3] for s in LC.WALK] and d[1:3] != LC.BATCH_SHAPE]
    assert all(N * C < 200 for _, N, C, _, _, _ in late) and len(late) <= 4, late


def test_pinned_share_table():
    """the table of docs/DESIGN_DETAIL.md ("the low-rank receiver"), at (200, 1024)"""
    N, C = LC.TABLE_SHAPE
    got = {}
    for r in (2, 8, 16, 24, 32):
        U, V, base = LC.build("random", N, C, r)
        got[r] = (W.pinned_share(U, V, base), W.pinned_share(U, V, None))
    print({r: (round(a, 3), round(b, 3)) for r, (a, b) in got.items()})
    assert all(a >= 0.90 for a, _ in got.values()) and all(b >= 0.80 for _, b in got.values())
    assert got[2][0] > got[16][0] > got[32][0]                     # the bound grows with the rank
    for name in LC.EXACT:
        for quant in (False, True):
            U, V, base = LC.build(name, N, C, 32, 0, quant)
            if quant:
                U, V = W.split_q(LC.q_packet(U, V), N, C, 32)
            assert W.pinned_share(U, V, base) == 1.0 and W.pinned_share(U, V, None) == 1.0
