"""The numpy contract of the INT2_MINMAX wire codec (tests/int2mm_contract.py) held to what is pinned: oracle.ref_np.sim_int2_minmax (itself
held to goldens captured from the reference, */i2mm/sim) wherever that is finite, code 0 and recv == min on constant channels, the float64
definition over the value domain of tests/_int2mm_cases.py - and the proof that every case of that domain holds what its `why` says."""
import numpy as np
import pytest

import _golden as G
import _int2mm_cases as IC
import int2mm_contract as I
from oracle import ref_np as R

F16, F64 = np.float16, np.float64
GOLD = "g3_g6_slowpath_codecs_eager.npz"


def _same_as_sim(d, what):
    pkt, recv = I.compress(d, None)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        sim = R.sim_int2_minmax(d)
    fin = np.isfinite(sim.astype(F64))
    assert np.array_equal(R.bits(recv)[fin], R.bits(sim)[fin]), what
    N, C = d.shape
    assert np.array_equal(R.bits(I.decompress(pkt, N, C)), R.bits(recv)), what + ": decompress(packet) != recv"
    return pkt, recv, fin


@pytest.mark.parametrize("shape", [(64, 256), (256, 1152)])
@pytest.mark.parametrize("seed", [42, 43, 44])
def test_contract_equals_the_pinned_function_on_the_golden_deltas(shape, seed):
    N, C = shape
    tag = f"{N}x{C}_s{seed}"
    assert f"{tag}/i2mm/sim" in G.manifest()[GOLD]          # (the larger shape is pinned by its sha256: G.check)
    x, base = G.inputs(GOLD, tag, seed, N, C)
    delta = (R.as_f16(x) - R.as_f16(base)).astype(F16)
    pkt, recv, fin = _same_as_sim(delta, tag)
    assert fin.all()
    G.check(GOLD, f"{tag}/i2mm/sim", R.bits(recv), "contract recv against the reference's sim_int2_minmax")
    pkt2, nb = I.residual_compress(x, base)
    assert np.array_equal(pkt, pkt2) and np.array_equal(R.bits(nb), R.bits((R.as_f16(base) + recv).astype(F16)))


@pytest.mark.parametrize("shape", [(4, 8), (8, 72), (68, 136), (132, 520), (256, 1152)])
@pytest.mark.parametrize("mag", [1e-4, 1.0, 300.0])
def test_contract_equals_the_pinned_function_on_random_inputs(shape, mag):
    N, C = shape
    rng = np.random.default_rng(N * 7919 + C)
    d = (rng.standard_normal((N, C)) * mag).astype(F16)
    d[:, 3] = d[0, 3]                       # constant channels: scale 0, NaN quotient
    d[:, C - 1] = 0.0
    pkt, recv, fin = _same_as_sim(d, f"{shape} x {mag}")
    const = [3, C - 1]
    assert not fin[:, const].any() and fin[:, [c for c in range(C) if c not in const]].all()
    q = I.unpack(pkt[:N * C // 8].view(np.uint8).reshape(N // 4, C))
    assert (q[:, const] == 0).all() and np.array_equal(R.bits(recv[:, const]), R.bits(d[:, const]))
    assert (pkt[N * C // 8:N * C // 8 + C][const] == 0).all()                     # scale 0


def test_packing_is_four_rows_per_byte_along_n():
    q = (np.arange(8 * 8).reshape(8, 8) * 7 % 4).astype(np.uint8)
    p = I.pack(q)
    assert p.shape == (2, 8) and np.array_equal(I.unpack(p), q)
    for k in range(2):
        for c in range(8):
            assert p[k, c] == q[4 * k, c] | q[4 * k + 1, c] << 2 | q[4 * k + 2, c] << 4 | q[4 * k + 3, c] << 6
    assert I.packet_halves(8, 72) * 2 == 8 * 72 // 4 + 4 * 72


def _params():
    return [pytest.param(N, C, n, id=f"{N}x{C}-{n}") for N, C in IC.ALL_SHAPES for n in IC.NAMES]


@pytest.mark.parametrize("N,C,case", _params())
def test_contract_against_the_float64_definition_over_the_value_domain(N, C, case):
    for rep in range(min(2, IC.reps(case, N, C))):
        x, base = IC.build(case, N, C, rep=rep)
        state = base
        for t in range(2):                  # the second round's residual is the first round's quantisation error
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                pkt, nb = I.residual_compress(x, state)
                rec = I.residual_decompress(pkt, state, N, C)
            assert np.array_equal(R.bits(rec), R.bits(nb))
            if case in IC.FINITE:
                I.check_f64(x, state, pkt, R.bits(nb))
            state = nb
    d, _ = IC.build(case, N, C, nobase=True)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        pkt, nb = I.residual_compress(d, None)
    if case in IC.FINITE:
        I.check_f64(d, None, pkt, R.bits(nb))


def test_every_case_holds_what_its_why_says():
    N, C = 68, 144
    qn = N * C // 8

    def parts(case, rep=0):
        x, base = IC.build(case, N, C, rep=rep)
        d = IC.V.delta(x, base)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            pkt, _ = I.compress(x, base)
        return d, I.unpack(pkt[:qn].view(np.uint8).reshape(N // 4, C)), pkt[qn:qn + C].view(F16), pkt[qn + C:].view(F16)
    seen = set()
    for rep in range(IC.reps("extremes-placed", N, C)):
        d, q, s, m = parts("extremes-placed", rep)
        rmin, rmax = IC.extreme_plan(N, C, rep)
        assert (d.argmin(axis=0) == rmin).all() and (d.argmax(axis=0) == rmax).all()
        seen |= set(rmin.tolist()) | set(rmax.tolist())
    assert seen >= set(IC.extreme_rows(N)) and {r % 4 for r in seen} == {0, 1, 2, 3} and set(range(64)) <= seen
    d, q, s, m = parts("constant-channels")
    assert s[0] == 0 and s[1] == 0 and (q[:, :2] == 0).all() and s[2] == 0 and set(np.unique(q[:, 2])) == {0, 3}
    d, q, s, m = parts("signed-zero-extremes")
    u = d.view(np.uint16)
    assert ((u[:, 0] == 0x8000).any() and (u[:, 0] == 0).any() and d[:, 0].min() == 0)
    d, q, s, m = parts("tiny")
    assert (s.astype(F64) < 2.0 ** -14).all() and (s > 0).any()
    d, q, s, m = parts("clamp-at-top")
    with np.errstate(divide="ignore", invalid="ignore"):
        quo = (d.astype(F64) - m.astype(F64)) / s.astype(F64)
    assert (quo[:, s > 0] >= 3.5).any() and np.isinf(quo).any() and (q[np.nan_to_num(quo, nan=0) >= 3.5] == 3).all()
    d, q, s, m = parts("wide")
    assert ((d.max(axis=0).astype(F64) - d.min(axis=0).astype(F64)) > 32768).all()
    d, q, s, m = parts("range-overflow")
    assert np.isinf(s.astype(F64)).sum() == 4
    d, q, s, m = parts("rint-ties")
    assert (s == 1.0).all() and (m == 0).all()
    ties = np.isin(d, np.array([0.5, 1.5, 2.5], F16))
    assert ties.any() and np.array_equal(q[ties], np.rint(d[ties].astype(F64)).astype(np.uint8)) and set(np.unique(q[ties])) == {0, 2}
    for t, lo, hi in ((0.5, 0, 1), (1.5, 1, 2), (2.5, 2, 3)):
        below, above = np.nextafter(F16(t), F16(0)), np.nextafter(F16(t), F16(4))
        assert (q[d == below] == lo).all() and (q[d == above] == hi).all() and (d == below).any() and (d == above).any()
