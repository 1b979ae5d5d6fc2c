"""The numpy contract of the MXFP4 wire codec (tests/mxfp4_contract.py; include/cfx.h "MXFP4") against the independent float64 witness
(tests/_mxfp4_f64_check.py) over every shape, value case and repetition of tests/_mxfp4_cases.py and over random inputs; the packet layout
byte for byte on a hand-written example; sender state == receiver state under error feedback.  CPU only."""
import numpy as np
import pytest

import _mxfp4_cases as MC
import _mxfp4_f64_check as F
import mxfp4_contract as M
from oracle import ref_np as R

F16 = np.float16


def _is_nan(b):
    return (b & 0x7FFF) > 0x7C00


# (the 16-item layer shape carries the random, edge and non-finite cases: its 52 224 blocks hold every planted block of the others at once)
_PARAMS = [(case, N, C) for case in MC.NAMES for N, C in MC.SHAPES] + [(case, *MC.LAYER16) for case in ("random", "edges", "nonfinite")]


@pytest.mark.parametrize("case,N,C", _PARAMS, ids=[f"{c}-{n}x{k}" for c, n, k in _PARAMS])
def test_contract_against_the_float64_witness(case, N, C):
    for rep in range(MC.reps(case, N, C)):
        for nobase in (False, True):
            x, base = MC.build(case, N, C, rep=rep, nobase=nobase)
            pkt, nb = M.residual_compress(x, base, True)
            assert pkt.dtype == np.uint16 and pkt.size == M.packet_halves(N, C) and 2 * pkt.size == N * C // 2 + N * C // 32
            F.check(x, base, pkt, R.bits(nb))
            rec = M.residual_decompress(pkt, base, N, C)
            gb, wb = R.bits(rec), R.bits(nb)
            assert np.array_equal(_is_nan(gb), _is_nan(wb)) and np.array_equal(gb[~_is_nan(wb)], wb[~_is_nan(wb)]), "receiver != sender"
            _, nb2 = M.residual_compress(x, base, False)
            F.check(x, base, pkt, R.bits(nb2), ef=False)
            if case in MC.FINITE:
                assert np.isfinite(nb.astype(np.float64)).all() and not (M.split(pkt, N, C)[1] == 0xFF).any()
                sb = M.split(pkt, N, C)[1]
                assert sb.min() >= 104 and sb.max() <= 140


def test_the_non_finite_cases_touch_only_their_blocks():
    for case in ("overflow", "nonfinite"):
        N, C = 5, 320
        x, base = MC.build(case, N, C)
        pkt, nb = M.residual_compress(x, base)
        sb = M.split(pkt, N, C)[1].reshape(-1)
        pl = MC.planted(case, N, C)
        assert set(np.nonzero(sb == 0xFF)[0]) == set(pl), (case, pl)
        nanblk = _is_nan(R.bits(nb)).reshape(-1, 32)
        assert nanblk[pl].all() and not np.delete(nanblk, pl, axis=0).any()


def test_every_case_plants_what_it_says():
    """the value cases reach the contract's corners: every scale byte from the clamp to the top, every code, ties on both sides"""
    seen_sb, seen_codes = set(), set()
    for case in MC.FINITE:
        for rep in range(MC.reps(case, 2, 192)):
            x, base = MC.build(case, 2, 192, rep=rep)
            c, sb = M.split(M.compress(x, base)[0], 2, 192)
            seen_sb |= set(sb.reshape(-1).tolist())
            seen_codes |= set(c.reshape(-1).tolist())
    assert seen_codes == set(range(16)) and {104, 140} <= seen_sb and len(seen_sb) >= 30, (sorted(seen_codes), sorted(seen_sb))


@pytest.mark.parametrize("seed", range(4))
def test_random_inputs(seed):
    rng = np.random.default_rng(seed)
    for N, C in MC.SHAPES[:6]:
        scale = np.exp(rng.standard_normal((N, 1)) * 2) * np.exp(rng.standard_normal((1, C)) * 2)
        with np.errstate(over="ignore"):
            base = rng.standard_normal((N, C)).astype(F16)
            x = np.clip(base.astype(np.float64) + rng.standard_t(3, (N, C)) * scale * 0.05, -60000, 60000).astype(F16)
        state = base
        for t in range(3):                                  # error feedback over rounds: the sender's state is the receiver's
            pkt, nb = M.residual_compress(x, state)
            F.check(x, state, pkt, R.bits(nb))
            assert np.array_equal(R.bits(M.residual_decompress(pkt, state, N, C)), R.bits(nb))
            state = nb


def test_packet_layout_byte_for_byte():
    d = np.zeros((1, 64), dtype=F16)
    d[0, :8] = [6, -6, 0.25, 0.75, -0.1, 1.5, 3, 4]                     # max 6: e = 2, X = 0, byte 127; y = |d|
    d[0, 32:38] = [1.0, 0.5, -0.25, 0.125, 0.0625, -1.0]               # max 1: e = 0, X = -2, byte 125; y = 4 |d|
    pkt, recv = M.compress(d, None)
    by = pkt.view(np.uint8)
    want = np.zeros(34, dtype=np.uint8)
    want[0:4] = [0xF7, 0x20, 0x38, 0x65]        # codes 7, 15 | 0 (tie 0.25 -> 0), 2 (tie 0.75 -> 1.0) | 8 (-0.1 -> -0), 3 | 5, 6
    want[16:19] = [0x46, 0x1A, 0xE0]            # codes 6, 4 | 10 (-0.25 -> -1 * 2^-2), 1 | 0 (tie 0.25 -> 0), 14
    want[32:34] = [127, 125]
    assert np.array_equal(by, want), (by.tolist(), want.tolist())
    wr = np.zeros((1, 64), dtype=F16)
    wr[0, :8] = [6, -6, 0, 1.0, -0.0, 1.5, 3, 4]
    wr[0, 32:38] = [1.0, 0.5, -0.25, 0.125, 0, -1.0]
    assert np.array_equal(R.bits(recv), R.bits(wr))
    assert np.array_equal(R.bits(M.decompress(pkt, 1, 64)), R.bits(wr))
    assert np.array_equal(M.unpack(M.pack(np.arange(128, dtype=np.uint8).reshape(2, 64) & 15)), np.arange(128, dtype=np.uint8).reshape(2, 64) & 15)
    assert M.packet_halves(544, 3072) * 2 == 544 * 3072 // 2 + 544 * 3072 // 32


def test_relative_error_is_what_the_issue_measured():
    """decode(encode(d)) on a (544, 3072) randn residual: relative Frobenius error 0.115 (the prototype's figure, to two digits)"""
    d = np.random.default_rng(0).standard_normal((544, 3072)).astype(F16)
    _, recv = M.compress(d, None)
    e = np.linalg.norm(recv.astype(np.float64) - d.astype(np.float64)) / np.linalg.norm(d.astype(np.float64))
    assert 0.105 < e < 0.125, e
