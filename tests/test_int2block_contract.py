"""The numpy contract of the block-scaled 2-bit wire codec (tests/int2block_contract.py; include/cfx.h "INT2_BLOCK") against the
independent witness (tests/_int2block_f64_check.py) over every shape, block size, element type, value case and repetition of
tests/_int2block_cases.py and over random inputs; the packet layout byte for byte on a hand-written example; the corners the value cases
are there for, worked out by hand; sender state == receiver state under error feedback; the error on the G12 drift against BINARY_BLOCK's
contract and the INT2 oracle.  CPU only."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import _int2block_cases as BK
import _int2block_f64_check as F
import bblock_contract as BB
import int2block_contract as M
from oracle import ref_np as R

F16 = np.float16
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

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
            assert pkt.dtype == np.uint16 and pkt.size == M.packet_halves(N, C, B) and 2 * pkt.size == N * C // 4 + 2 * N * C // B
            F.check(x, base, pkt, B, nb, bf16=bf)
            assert np.array_equal(M.recon(pkt, base, N, C, B, bf), nb), "receiver != sender"
            pkt2, nb2 = M.step(x, base, B, bf, ef=False)
            assert np.array_equal(pkt2, pkt)
            F.check(x, base, pkt2, B, nb2, ef=False, bf16=bf)


def test_the_cases_plant_what_they_name():
    """the value cases reach the corners they are there for: magnitude bits of both kinds, a saturated level, a zero small level"""
    for B in BK.BLOCKS:
        N, C = 17, 384
        x, _ = BK.build("saturate", N, C, B, nobase=True)
        codes, s = M.split(M.step(x, None, B, False)[0], N, C, B)
        assert (s.astype(np.float64) > 32752).any() and (R.unpack_int2(codes) & 1).any()
        x, _ = BK.build("odd-scale", N, C, B, nobase=True)
        s = M.split(M.step(x, None, B, False)[0], N, C, B)[1]
        assert (R.bits(s) == 1).any() and ((R.bits(s) < 0x800) & (R.bits(s) % 2 == 1)).sum() >= 8
        x, _ = BK.build("all-equal", N, C, B, nobase=True)
        codes, s = M.split(M.step(x, None, B, False)[0], N, C, B)
        mags = (R.unpack_int2(codes) & 1).reshape(-1, B)
        same = (x.reshape(-1, B) & 0x7FFF == R.bits(s).reshape(-1, 1)).all(axis=1)
        assert same.sum() >= 8 and not mags[same].any()


def test_shape_rule_and_sizes():
    for B in BK.BLOCKS:
        for N, C in ((1, 64), (1, 128), (3, 128), (5, 192), (17, 384), (33, 1152), (129, 3072), (544, 3072)):
            assert M.shape_ok(N, C, B) == (C % max(B, 64) == 0)
        assert not M.shape_ok(4, 32, B) and not M.shape_ok(0, 128, B) and not M.shape_ok(4, 96, B)
    assert not M.shape_ok(4, 128, 16) and not M.shape_ok(4, 256, 256) and not M.shape_ok(4, 128, 0)
    assert M.packet_bytes(544, 3072, 32) * 8 == 544 * 3072 * 2.5 and M.packet_bytes(544, 3072, 64) * 8 == 544 * 3072 * 2.25
    assert M.packet_bytes(544, 3072, 128) * 8 == 544 * 3072 * 2.125


def test_packet_layout_byte_for_byte():
    d = np.zeros((1, 128), dtype=F16)
    d[0, :8] = [1, -1, 2, -2, 0.0, -0.0, 4, -4]                         # codes 3,1,3,1 | 2,2,3,1: bytes 0x77, 0x7A; the block's sum 14
    d[0, 64:72] = [-8, -8, -8, -8, 8, 8, 8, 8]                          # codes 1,1,1,1 | 3,3,3,3: 0x55, 0xFF; sum 64
    d[0, 127] = -32                                                     # byte 31: 2,2,2,1 = 0x6A; sum 64 + 32 = 96
    for B, scales in ((32, [14 / 32, 0, 2, 1]), (64, [14 / 64, 96 / 64]), (128, [110 / 128])):
        pkt, recv = M.compress(d, None, B)
        by = pkt.view(np.uint8)
        want = np.full(32, 0xAA, dtype=np.uint8)                        # a +0 has sign 1 and no magnitude bit: code 2
        want[0], want[1], want[16], want[17], want[31] = 0x77, 0x7A, 0x55, 0xFF, 0x6A
        assert np.array_equal(by[:32], want), (B, [hex(v) for v in by[:32]])
        assert np.array_equal(by[32:].view(F16), np.array(scales, dtype=F16)), (B, by[32:].view(F16))
        s = np.repeat(np.array(scales, dtype=np.float64), B)
        a = np.abs(d[0].astype(np.float64))
        wr = (np.where(np.signbit(d[0]) & (d[0] != 0), -1.0, 1.0) * np.where(a > s, 2 * s, 0.5 * s)).astype(F16)    # (exact here)
        assert np.array_equal(R.bits(recv[0]), R.bits(wr))
        assert np.array_equal(R.bits(M.decode(pkt, 1, 128, B)), R.bits(recv))


@pytest.mark.parametrize("B", BK.BLOCKS)
def test_the_corners_by_hand(B):
    W = max(B, 64) * 2
    u = lambda *a: np.asarray(a, dtype=np.uint16).view(F16)          # noqa: E731

    def enc(v):
        """block 0 of a (1, W) tensor = v -> (scale bits, codes of the block, recv bits of the block)"""
        d = np.zeros((1, W), dtype=F16)
        d[0, :B] = v
        pkt, recv = M.compress(d, None, B)
        codes, s = M.split(pkt, 1, W, B)
        return int(R.bits(s)[0, 0]), R.unpack_int2(codes)[0, :B], R.bits(recv)[0, :B]

    z = np.zeros(B, dtype=F16)
    # zero blocks of either sign: scale +0, code 2 (sign 1, no magnitude), recv +0 - for -0 too
    for v in (z, -z):
        s, c, r = enc(v)
        assert s == 0 and (c == 2).all() and not r.any()
    # a receiver's +0 / -0 by the sign bit where s == 0 (no sender makes code 0 there; a receiver decodes what it is given)
    pkt = np.zeros(M.packet_halves(1, W, B), dtype=np.uint16)
    pkt.view(np.uint8)[0] = 0b10_00_11_01
    assert R.bits(M.decode(pkt, 1, W, B))[0, :4].tolist() == [0x8000, 0, 0x8000, 0]
    # every |d| equal: s is that value, the compare is strict, nothing is sent large; recv = +-0.5 s
    v = np.where(np.arange(B) % 3 == 0, -1.5, 1.5).astype(F16)
    s, c, r = enc(v)
    assert s == R.bits(F16(1.5)) and np.array_equal(c, np.where(np.arange(B) % 3 == 0, 0, 2))
    assert np.array_equal(r, R.bits(np.where(np.arange(B) % 3 == 0, -0.75, 0.75).astype(F16)))
    # one element exactly at s, its fp16 neighbours beside it: 0x3C10 - 1, + 1 keep the mean at 0x3C10
    v = np.full(B, 0x3C10, dtype=np.uint16)
    v[1], v[2] = 0x3C11, 0x3C0F | 0x8000
    s, c, r = enc(v.view(F16))
    assert s == 0x3C10 and c[:4].tolist() == [2, 3, 0, 2]
    assert r[:3].tolist() == [0x3810, 0x4010, 0xB810]                 # 0.5 s, 2 s, -0.5 s: the exponent moves, the significand stays
    # subnormal and lowest-binade scales with an odd significand: 0.5 s is a tie and goes to even; s = 2^-24: small is 0, the sign stays
    for a, small in ((1, 0), (3, 2), (5, 2), (7, 4), (0x3FF, 0x200), (0x3FD, 0x1FE), (0x401, 0x200), (0x403, 0x202), (0x7FF, 0x400), (0x801, 0x401)):
        v = np.full(B, a, dtype=np.uint16)
        v[1] |= 0x8000
        s, c, r = enc(v.view(F16))
        assert s == a and r[0] == small and r[1] == (small | 0x8000) and c[0] == 2 and c[1] == 0, (a, s, r[:2])
    # a block of +-65504: s = 65504, no magnitude bit, recv = +-32752
    s, c, r = enc((np.where(np.arange(B) % 2, -1, 1) * 65504.0).astype(F16))
    assert s == 0x7BFF and set(c.tolist()) == {0, 2} and set(r.tolist()) == {0x77FF, 0xF7FF}
    # 2 s past fp16: large is 65504, never inf.  49152 everywhere and one -65504: s = fp16(49152 + 16352 / B)
    v = np.full(B, 49152.0, dtype=F16)
    v[5] = -65504.0
    s, c, r = enc(v)
    assert 0x7A00 < s < 0x7BFF and c[5] == 1 and r[5] == 0xFBFF and c[4] == 2 and r[4] == R.bits(F16(0.5) * u(s))[0]
    sm, lg = M.levels(u(0x77FE, 0x77FF, 0x7800, 0x7BFF))
    assert R.bits(lg).tolist() == [0x7BFE, 0x7BFF, 0x7BFF, 0x7BFF] and R.bits(sm).tolist() == [0x73FE, 0x73FF, 0x7400, 0x77FF]
    # the fp32 conversion of the sum rounds first (bblock's corner): 2^24 + 2^13 + 1 units is a tie in fp32 and goes to the even side
    lo = F16(1.0 / B)
    v = z.copy()
    v[:3] = [1.0, np.ldexp(1.0, -11), u(1)[0]]
    assert enc(v)[0] == R.bits(lo)


def test_nothing_leaks_between_blocks():
    """a block of tiny values between blocks of huge ones, and the last block of a row against the first of the next: every scale is its
    own block's mean, and every level is a level of its own block's scale"""
    for N, C in ((3, 128), (5, 192), (17, 384)):
        for B in BK.blocks_of(N, C):
            x, _ = BK.build("neighbours", N, C, B, nobase=True)
            d = x.view(F16)
            pkt, recv = M.compress(d, None, B)
            s = M.split(pkt, N, C, B)[1].astype(np.float64).reshape(-1)
            a = np.abs(d.astype(np.float64)).reshape(-1, B)
            assert ((s >= a.min(axis=1)) & (s <= a.max(axis=1))).all()
            big = s > 1000
            assert big.any() and (~big).any() and (s[~big] < 1e-5).all() and (big[1:] != big[:-1]).all()
            r = np.abs(recv.astype(np.float64)).reshape(-1, B)
            assert (r[~big] < 1e-4).all() and (r[big] > 500).all()


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


def test_levels_are_int2s_below_the_saturation():
    """wherever 2 s stays in fp16 the two levels are R.int2_levels' with the block scale as the threshold, bit for bit"""
    s = np.arange(0, 0x7800, dtype=np.uint16).view(F16).reshape(1, -1)                  # every scale up to 32752
    for code in range(4):
        idx = np.full(s.shape, code, dtype=np.uint8)
        assert np.array_equal(R.bits(M.recv_of(idx, s, 1)), R.bits(R.int2_levels(idx, s)))


# ---- quality on the G12 drift --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _g12(seed):
    """the G12 inputs of one tensor (bits, 28 steps) and the INT2 oracle's error per step on them (step 0 is the warm-up)"""
    spec = importlib.util.spec_from_file_location("make_golden_quality", os.path.join(REPO, "tests", "golden", "make_golden_quality.py"))
    mq = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mq)
    assert (mq.N, mq.C) == (128, 3072)
    xs = [R.bits(x.numpy()).reshape(mq.N, mq.C).copy() for x in mq.drift(seed, 28)]
    return xs, _trace(xs, lambda x, st: R.bits(R.residual_compress("int2", x, st, 0, True)[1]))


def _trace(xs, step):
    """relative error of the error-feedback state against the input, per compressed step"""
    st, out = xs[0].copy(), []
    for x in xs[1:]:
        st = np.ascontiguousarray(step(x, st)).reshape(x.shape).copy()
        x64 = x.view(F16).astype(np.float64)
        out.append(np.linalg.norm(st.view(F16).astype(np.float64) - x64) / np.linalg.norm(x64))
    return np.array(out)


@pytest.mark.parametrize("B", BK.BLOCKS)
@pytest.mark.parametrize("seed", [4242, 4243], ids=["K", "V"])
def test_g12_error_below_binary_block_and_at_int2(seed, B):
    """The contract's error-feedback trace on the G12 drift inputs ((128, 3072), 28 steps; K: seed 4242, V: 4243).  On EVERY step the
    error is strictly below BINARY_BLOCK's contract at the same block size, and at most 1.02 x the INT2 oracle's: the codec has INT2's
    levels, so it has INT2's error (measured worst ratio: 1.0056 on K, 1.0040 on V) - the margin covers nothing but that."""
    xs, e_int2 = _g12(seed)
    e_own = _trace(xs, lambda x, st: M.step(x, st, B, False)[1])
    e_bb = _trace(xs, lambda x, st: BB.step(x, st, B, False)[1])
    ratio = e_own / e_int2
    print(f"seed {seed} B {B}: int2-block mean {e_own.mean():.4f} max {e_own.max():.4f}; binary-block mean {e_bb.mean():.4f}; "
          f"int2 mean {e_int2.mean():.4f} max {e_int2.max():.4f}; worst ratio to int2 {ratio.max():.4f}")
    assert len(e_own) == 27
    assert (e_own < e_bb).all(), (e_own, e_bb)
    assert (ratio <= 1.02).all(), ratio.max()
