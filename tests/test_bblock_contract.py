"""The numpy contract of the block-scaled 1-bit wire codec (tests/bblock_contract.py; include/cfx.h "BINARY_BLOCK") against the
independent witness (tests/_bblock_f64_check.py) over every shape, block size, element type, value case and repetition of
tests/_bblock_cases.py and over random inputs; the packet layout byte for byte on a hand-written example; the corners the value cases are
there for, worked out by hand; sender state == receiver state under error feedback.  CPU only."""
import numpy as np
import pytest

import _bblock_cases as BK
import _bblock_f64_check as F
import bblock_contract as M
from oracle import ref_np as R

F16 = np.float16

_PARAMS = [(case, N, C, B, bf) for bf in (False, True) for case in BK.cases_for(bf) for N, C in BK.SHAPES for B in BK.blocks_of(N, C)]
_PARAMS += [("random", *BK.BIG, B, bf) for bf in (False, True) for B in BK.BLOCKS]


def _id(p):
    case, N, C, B, bf = p
    return f"{case}-{N}x{C}-B{B}-{'bf16' if bf else 'fp16'}"


@pytest.mark.parametrize("case,N,C,B,bf", _PARAMS, ids=[_id(p) for p in _PARAMS])
def test_contract_against_the_witness(case, N, C, B, bf):
    for rep in range(BK.reps(case, N, C, B)):
        for nobase in (False, True):
            x, base = BK.build(case, N, C, B, bf, rep=rep, nobase=nobase)
            pkt, nb = M.step(x, base, B, bf)
            assert pkt.dtype == np.uint16 and pkt.size == M.packet_halves(N, C, B) and 2 * pkt.size == N * C // 8 + 2 * N * C // B
            F.check(x, base, pkt, B, nb, bf16=bf)
            assert np.array_equal(M.recon(pkt, base, N, C, B, bf), nb), "receiver != sender"
            pkt2, nb2 = M.step(x, base, B, bf, ef=False)
            assert np.array_equal(pkt2, pkt)
            F.check(x, base, pkt2, B, nb2, ef=False, bf16=bf)


def test_shape_rule_and_sizes():
    for B in BK.BLOCKS:
        for N, C in ((1, 64), (1, 128), (3, 128), (5, 192), (17, 384), (33, 1152), (129, 3072), (544, 3072)):
            assert M.shape_ok(N, C, B) == (C % max(B, 64) == 0)
        assert not M.shape_ok(4, 32, B) and not M.shape_ok(0, 128, B) and not M.shape_ok(4, 96, B)
    assert not M.shape_ok(4, 128, 16) and not M.shape_ok(4, 256, 256) and not M.shape_ok(4, 128, 0)
    assert M.packet_bytes(544, 3072, 32) * 8 == 544 * 3072 * 1.5 and M.packet_bytes(544, 3072, 64) * 8 == 544 * 3072 * 1.25
    assert M.packet_bytes(544, 3072, 128) * 8 == 544 * 3072 * 1.125


def test_packet_layout_byte_for_byte():
    d = np.zeros((1, 128), dtype=F16)
    d[0, :8] = [1, -1, 2, -2, 0.0, -0.0, 4, -4]                         # bits 1,0,1,0,1,1,1,0 = 0x75; the block's sum 14
    d[0, 64:72] = [-8, -8, -8, -8, 8, 8, 8, 8]                          # 0xF0; sum 64
    d[0, 127] = -32                                                     # byte 15: 0x7F; sum 64 + 32 = 96
    for B, scales in ((32, [14 / 32, 0, 2, 1]), (64, [14 / 64, 96 / 64]), (128, [110 / 128])):
        pkt, recv = M.compress(d, None, B)
        by = pkt.view(np.uint8)
        want = np.full(16, 0xFF, dtype=np.uint8)
        want[0], want[8], want[15] = 0x75, 0xF0, 0x7F
        assert np.array_equal(by[:16], want), (B, by[:16].tolist())
        assert np.array_equal(by[16:].view(F16), np.array(scales, dtype=F16)), (B, by[16:].view(F16))
        s = np.repeat(np.array(scales, dtype=F16), B)
        wr = np.where(np.signbit(d[0]) & (d[0] != 0), -s, s).astype(F16)
        wr[5] = s[5]                                                    # -0 has bit 1: +s
        assert np.array_equal(R.bits(recv[0]), R.bits(wr))
        assert np.array_equal(R.bits(M.decode(pkt, 1, 128, B)), R.bits(recv))


@pytest.mark.parametrize("B", BK.BLOCKS)
def test_the_corners_by_hand(B):
    def s_of(v):
        d = np.zeros((1, max(B, 64) * 2), dtype=F16)
        d[0, :B] = v
        return R.bits(M.split(M.compress(d, None, B)[0], 1, d.shape[1], B)[1])[0, 0]
    u = lambda *a: np.asarray(a, dtype=np.uint16).view(F16)          # noqa: E731
    z = np.zeros(B, dtype=F16)
    # zero blocks of either sign: scale +0; recv +0 for -0 too (its bit is 1)
    assert s_of(z) == 0 and s_of(-z) == 0
    d = np.zeros((1, 256), dtype=F16)
    d[0, :B] = -z
    pkt, recv = M.compress(d, None, B)
    assert not R.bits(recv).any() and (pkt.view(np.uint8)[:32] == 0xFF).all()
    # subnormal sums: B/2 units is the tie between 0 and 2^-24 (even: 0), one more rounds up, 3B/2 is the tie between 1 and 2 (even: 2)
    one = u(1)[0]
    for total, want in ((1, 0), (B // 2 - 1, 0), (B // 2, 0), (B // 2 + 1, 1), (B, 1), (3 * B // 2 - 1, 1), (3 * B // 2, 2), (5 * B // 2, 2), (5 * B // 2 + 1, 3)):
        v = z.copy()
        k, r = divmod(total, B)
        v[:] = u(k)[0]
        v[:r] = u(k + 1)[0]
        assert s_of(v) == want, (B, total, s_of(v), want)
    assert one == np.ldexp(1.0, -24)
    # every element 65504: the mean is 65504
    assert s_of(np.full(B, -65504, dtype=F16)) == 0x7BFF
    # half-way means go to the even neighbour
    for a in (0x3C00, 0x3C01, 0x03FF, 0x7BFE):
        v = np.where(np.arange(B) % 2, a + 1, a).astype(np.uint16).view(F16)
        assert s_of(v) == (a if a % 2 == 0 else a + 1), hex(a)
    # the fp32 conversion of the sum rounds first: 2^24 + 2^13 + 1 units is a tie in fp32, goes to the even 2^24 + 2^13, and that is the
    # tie between two fp16 means, which goes to the even one - one rounding of the exact mean would have gone up
    lo, hi = F16(1.0 / B), u(R.bits(F16(1.0 / B)) + 1)[0]
    v = z.copy()
    v[:2] = [1.0, np.ldexp(1.0, -11)]
    assert s_of(v) == R.bits(lo)
    v[2] = one
    assert s_of(v) == R.bits(lo)
    v[3] = one
    assert s_of(v) == R.bits(hi)                      # + 2 units: one ulp of fp32 above the tie
    # one nonzero element: the scale is that element over B, exactly
    v = z.copy()
    v[B - 1] = -48.0
    assert s_of(v) == R.bits(F16(48.0 / B))


def test_nothing_leaks_between_blocks():
    """a block of tiny values between blocks of huge ones, and the last block of a row against the first of the next: every scale is its
    own block's mean"""
    for N, C in ((3, 128), (5, 192), (17, 384)):
        for B in BK.blocks_of(N, C):
            x, _ = BK.build("neighbours", N, C, B, nobase=True)
            d = x.view(F16)
            s = M.split(M.compress(d, None, B)[0], N, C, B)[1].astype(np.float64).reshape(-1)
            a = np.abs(d.astype(np.float64)).reshape(-1, B)
            assert ((s >= a.min(axis=1)) & (s <= a.max(axis=1))).all()
            big = s > 1000
            assert big.any() and (~big).any() and (s[~big] < 1e-5).all() and (big[1:] != big[:-1]).all()


@pytest.mark.parametrize("seed", range(3))
def test_random_inputs_over_rounds_of_error_feedback(seed):
    rng = np.random.default_rng(seed)
    for N, C in BK.SHAPES:
        for B in BK.blocks_of(N, C):
            scale = np.exp(rng.standard_normal((N, 1)) * 2) * np.exp(rng.standard_normal((1, C)) * 2)
            base = rng.standard_normal((N, C)).astype(F16)
            x = np.clip(base.astype(np.float64) + rng.standard_t(3, (N, C)) * scale * 0.05, -30000, 30000).astype(F16)
            for bf in (False, True):
                xs, state = (R.bits(x), R.bits(base)) if not bf else (M.BC.f32_to_bf16(x.astype(np.float32)), M.BC.f32_to_bf16(base.astype(np.float32)))
                for t in range(3):                              # the sender's state is the receiver's
                    pkt, nb = M.step(xs, state, B, bf)
                    F.check(xs, state, pkt, B, nb, bf16=bf)
                    assert np.array_equal(M.recon(pkt, state, N, C, B, bf), nb)
                    state = nb


def test_a_bf16_senders_packet_is_an_fp16_packet():
    """the wire does not say what its sender's activations were: an fp16 receiver reconstructs a bf16 sender's packet onto its fp16 state"""
    N, C, B = 5, 192, 64
    x, base = BK.build("random", N, C, B, bf16=True)
    pkt, _ = M.step(x, base, B, True)
    d16 = M.BC.delta(x, base)
    pkt16, recv = M.compress(d16, None, B)
    assert np.array_equal(pkt, pkt16)
    state16 = np.random.default_rng(1).standard_normal((N, C)).astype(F16)
    assert np.array_equal(R.bits(M.residual_decompress(pkt, state16, N, C, B)), R.bits((state16 + recv).astype(F16)))


def test_relative_error_of_a_gaussian_residual():
    """decode(encode(d)) on a (544, 3072) randn residual: a sign compressor with the block's mean magnitude leaves a relative Frobenius
    error of sqrt(1 - 2 / pi) = 0.603, whatever the block size"""
    d = np.random.default_rng(0).standard_normal((544, 3072)).astype(F16)
    for B in BK.BLOCKS:
        _, recv = M.compress(d, None, B)
        e = np.linalg.norm(recv.astype(np.float64) - d.astype(np.float64)) / np.linalg.norm(d.astype(np.float64))
        assert abs(e - np.sqrt(1 - 2 / np.pi)) < 0.01, (B, e)
