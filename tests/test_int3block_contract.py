"""The numpy contract of the block-scaled 3-bit wire codec (tests/int3block_contract.py; include/cfx.h "INT3_BLOCK") against the
independent witness (tests/_int3block_f64_check.py) over every shape, block size, element type, value case and repetition of
tests/_int3block_cases.py and over random inputs; the packet layout byte for byte on a hand-written example; the corners the value cases
are there for, worked out by hand; sender state == receiver state under error feedback; the error on the G12 drift against INT2_BLOCK's
and MXFP4's contracts.  CPU only."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import _int3block_cases as BK
import _int3block_f64_check as F
import int2block_contract as I2
import int3block_contract as M
import mxfp4_contract as MX
from oracle import ref_np as R

F16 = np.float16
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_PARAMS = [(case, N, C, B, bf) for bf in (False, True) for case in BK.cases_for(bf) for N, C in BK.SHAPES + BK.INHERITED for B in BK.blocks_of(N, C)]
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
            assert pkt.dtype == np.uint16 and pkt.size == M.packet_halves(N, C, B) and 2 * pkt.size == 3 * N * C // 8 + 2 * N * C // B
            F.check(x, base, pkt, B, nb, bf16=bf)
            assert np.array_equal(M.recon(pkt, base, N, C, B, bf), nb), "receiver != sender"
            pkt2, nb2 = M.step(x, base, B, bf, ef=False)
            assert np.array_equal(pkt2, pkt)
            F.check(x, base, pkt2, B, nb2, ef=False, bf16=bf)


def _mags_scales(x, N, C, B):
    hi, lo, s = M.split(M.step(x, None, B, False)[0], N, C, B)
    return M.unpack(hi, lo)[1].reshape(-1, B), R.bits(s).reshape(-1)


def test_the_cases_plant_what_they_name():
    """the value cases reach the corners they are there for"""
    for B in BK.BLOCKS:
        N, C = 129, 128
        # every threshold of a block with an element AT it (not sent above it) and elements one fp16 step to either side (above: sent above)
        for case in ("at-thresholds", "subnormal-thresholds"):
            x, _ = BK.build(case, N, C, B, nobase=True)
            mags, sb = _mags_scales(x, N, C, B)
            a = (x & 0x7FFF).reshape(-1, B).astype(np.int64)
            hits = 0
            for blk in range(sb.size):
                thr = [int(R.bits(t)[0]) for t in M.thresholds(np.array([sb[blk]], dtype=np.uint16).view(F16))]
                if not all((a[blk] == t).any() and (a[blk] == t + 1).any() for t in thr):
                    continue
                hits += 1
                for k, t in enumerate(thr):
                    assert (mags[blk][a[blk] == t] <= k).all() and (mags[blk][a[blk] == t + 1] >= k + 1).all()
            assert hits >= (18 if case == "at-thresholds" else 11), (case, B, hits)
        assert (sb == 1).any() and (sb == 2).any()
        one = (a == 1).all(axis=1)
        assert one.any() and not mags[one].any()                 # a block of 1 unit everywhere: s = t_0 = 1 unit, the compare is strict
        # all four magnitudes occur; a saturated top level with mag 3 present; saturated thresholds with mag 3, then 2, absent
        x, _ = BK.build("saturate-levels", N, C, B, nobase=True)
        mags, sb = _mags_scales(x, N, C, B)
        s = sb.view(F16).astype(np.float64)
        top = (s * 3.375 > 65504) & (s * 2.625 < 65504)
        assert top.any() and (mags[top] == 3).any(axis=1).sum() >= 3
        t2 = (s * 2.625 > 65504) & (s * 1.5 < 65504)
        assert t2.sum() >= 2 and (mags[t2].max(axis=1) == 2).all()
        t1 = s * 1.5 > 65504
        assert t1.sum() >= 2 and (mags[t1].max(axis=1) == 1).all()
        x, _ = BK.build("random", N, C, B, nobase=True)
        assert set(np.unique(_mags_scales(x, N, C, B)[0]).tolist()) == {0, 1, 2, 3}


def test_shape_rule_and_sizes():
    for B in BK.BLOCKS:
        for N, C in ((1, 64), (1, 128), (3, 192), (5, 320), (4, 2112), (129, 128), (129, 3072), (544, 3072)):
            assert M.shape_ok(N, C, B) == (C % max(B, 64) == 0)
        assert not M.shape_ok(4, 32, B) and not M.shape_ok(0, 128, B) and not M.shape_ok(4, 96, B)
    assert not M.shape_ok(4, 128, 16) and not M.shape_ok(4, 256, 256) and not M.shape_ok(4, 128, 0)
    assert M.packet_bytes(544, 3072, 32) * 8 == 544 * 3072 * 3.5 and M.packet_bytes(544, 3072, 64) * 8 == 544 * 3072 * 3.25
    assert M.packet_bytes(544, 3072, 128) * 8 == 544 * 3072 * 3.125


def test_packet_layout_byte_for_byte():
    d = np.zeros((1, 128), dtype=F16)
    # block sums 32 / 32 / 32 (B = 32: s = 1 in blocks 0 and 2, 0 in 1 and 3), 32 and 64 (B = 64: s = 0.5, 1), 96 (B = 128: s = 0.75)
    d[0, :8] = [4, -4, 2, -2, 1, -1, 0.5, -0.5]                         # 15 of the 32; the rest of block 0 below
    d[0, 8:16] = [3, -3, 1.5, -1.5, 0.75, -0.75, 0.25, 0.0]             # 10.75
    d[0, 16:24] = [2.625, -2.625, 0.5, 0.5, -0.0, 0, 0, 0]              # 6.25: together 32
    d[0, 64:72] = [-8, -8, 8, 8, 0, 0, 0, 0]                            # 32
    d[0, 120:128] = [0, 0, 0, 0, 0, 0, 16, -16]                         # 32
    for B, scales in ((32, [1, 0, 1, 1]), (64, [0.5, 1]), (128, [0.75])):
        pkt, recv = M.compress(d, None, B)
        by = pkt.view(np.uint8)
        s = np.repeat(np.array(scales, dtype=np.float64), B)
        a = np.abs(d[0].astype(np.float64))
        mag = (a > 0.75 * s).astype(int) + (a > 1.5 * s) + (a > 2.625 * s)          # (every product is an fp16 value here)
        sign = (~(np.signbit(d[0]) & (d[0] != 0))).astype(int)          # -0 is not below zero: 1
        code = sign * 2 + mag // 2
        want_hi = [int(sum(int(code[4 * j + i]) << (2 * i) for i in range(4))) for j in range(32)]
        want_lo = [int(sum(int(mag[8 * j + i] & 1) << i for i in range(8))) for j in range(16)]
        assert by[:32].tolist() == want_hi, (B, [hex(v) for v in by[:32]])
        assert by[32:48].tolist() == want_lo, (B, [hex(v) for v in by[32:48]])
        assert np.array_equal(by[48:].view(F16), np.array(scales, dtype=F16)), (B, by[48:].view(F16))
        assert by.size == 48 + 2 * 128 // B
        lv = np.array([0.375, 1.125, 1.875, 3.375])
        wr = (np.where(sign == 1, 1.0, -1.0) * lv[mag] * s).astype(F16)             # (exact here)
        assert np.array_equal(R.bits(recv[0]), R.bits(wr))
        assert np.array_equal(R.bits(M.decode(pkt, 1, 128, B)), R.bits(recv))
    # B = 32, written out: element 0 (4 > 2.625: mag 3, +) .. element 7 (-0.5 <= 0.75: mag 0, -); hi bytes 3,1,3,1 -> 0x77; 2,0,2,0 -> 0x22;
    # lo byte: mags 3,3,2,2,1,1,0,0 -> bits 1,1,0,0,1,1,0,0 -> 0x33
    by = M.compress(d, None, 32)[0].view(np.uint8)
    assert by[0] == 0x77 and by[1] == 0x22 and by[32] == 0x33
    # elements 16, 17 are +-2.625 = t_2 exactly: mag 2, lo bit 0; 18, 19 are 0.5: mag 0; 20 is -0: sign 1 -> hi codes 3,1,2,2 | 2,2,2,2
    assert by[4] == 0b10_10_01_11 and by[5] == 0xAA and by[34] == 0x00


@pytest.mark.parametrize("B", BK.BLOCKS)
def test_the_corners_by_hand(B):
    W = max(B, 64) * 2
    u = lambda *a: np.asarray(a, dtype=np.uint16).view(F16)          # noqa: E731

    def enc(v):
        """block 0 of a (1, W) tensor = v -> (scale bits, signs, mags, recv bits of the block)"""
        d = np.zeros((1, W), dtype=F16)
        d[0, :B] = v
        pkt, recv = M.compress(d, None, B)
        hi, lo, s = M.split(pkt, 1, W, B)
        sg, mg = M.unpack(hi, lo)
        return int(R.bits(s)[0, 0]), sg[0, :B], mg[0, :B], R.bits(recv)[0, :B]

    z = np.zeros(B, dtype=F16)
    # zero blocks of either sign: scale +0, sign 1, mag 0, recv +0 - for -0 too
    for v in (z, -z):
        s, sg, mg, r = enc(v)
        assert s == 0 and (sg == 1).all() and not mg.any() and not r.any()
    # a receiver's +0 / -0 by the sign bit where s == 0, whatever the magnitude bits say
    pkt = np.zeros(M.packet_halves(1, W, B), dtype=np.uint16)
    pkt.view(np.uint8)[0] = 0b10_00_11_01
    pkt.view(np.uint8)[W // 4] = 0b0101
    assert R.bits(M.decode(pkt, 1, W, B))[0, :4].tolist() == [0x8000, 0, 0x8000, 0]
    # every |d| equal: s is that value, above t_0 = 0.75 s and not above t_1: mag 1 everywhere, recv = +-1.125 s
    v = np.where(np.arange(B) % 3 == 0, -2.0, 2.0).astype(F16)
    s, sg, mg, r = enc(v)
    assert s == R.bits(F16(2.0)) and (mg == 1).all() and np.array_equal(sg, np.where(np.arange(B) % 3 == 0, 0, 1))
    assert np.array_equal(r, R.bits(np.where(np.arange(B) % 3 == 0, -2.25, 2.25).astype(F16)))
    # s = 1 exactly (the rest of the block at 1 - 11.625 / (B - 12) ... kept simple: 9 planted elements and a fill that makes the sum B):
    # elements exactly at 0.75, 1.5, 2.625 are NOT above them; one fp16 step up is
    v = np.full(B, 0, dtype=np.uint16)
    v[:9] = [0x3A00, 0x3A01, 0x39FF, 0x3E00, 0x3E01, 0x3DFF, 0x4140, 0x4141, 0x413F]       # 3 x (0.75 + 1.5 + 2.625) = 14.625
    rest = (B - 14.625) / (B - 9)                                                           # 0.7554.., 0.8977.., 0.9527..: not fp16 values
    fill = np.full(B - 9, np.floor(rest * 2048) / 2048)                                    # multiples of the binade's ulp 2^-11 ...
    k = int(round((B - 14.625 - fill.sum()) * 2048))
    fill[:k] += 1 / 2048                                                                    # ... k of them one ulp up: the sum is B exactly
    v[9:] = R.bits(fill.astype(F16))
    assert v.view(F16).astype(np.float64).sum() == B
    s, sg, mg, r = enc(v.view(F16))
    assert s == 0x3C00 and mg[:9].tolist() == [0, 1, 0, 1, 2, 1, 2, 3, 2]
    assert r[:9].tolist() == [R.bits(F16(x)) for x in (0.375, 1.125, 0.375, 1.125, 1.875, 1.125, 1.875, 3.375, 1.875)]
    # s = 2^-24: t = fp16(0.75), fp16(1.5), fp16(2.625) units = 1, 2 (a tie, to even), 3; l = 0, 1, 2, 3 units
    t = M.thresholds(u(1))
    assert [int(R.bits(x)[0]) for x in t] == [1, 2, 3] and [int(R.bits(x)[0]) for x in M.levels(u(1))] == [0, 1, 2, 3]
    v = np.zeros(B, dtype=np.uint16)
    v[:5] = [1, 2, 3, 4 | 0x8000, 0]                              # sum 10 ... the rest ones: sum B + 5 - rounds to s = 1 unit for every B >= 32
    v[5:] = 1
    s, sg, mg, r = enc(v.view(F16))
    assert s == 1 and mg[:6].tolist() == [0, 1, 2, 3, 0, 0] and r[:5].tolist() == [0, 1, 2, 3 | 0x8000, 0]
    # colliding thresholds: s = 2 units: t = 1.5 -> 2, 3, 5.25 -> 5;  s = 3 units: 2.25 -> 2, 4.5 -> 4 (tie, even), 7.875 -> 8
    assert [int(R.bits(x)[0]) for x in M.thresholds(u(2))] == [2, 3, 5] and [int(R.bits(x)[0]) for x in M.thresholds(u(3))] == [2, 4, 8]
    assert [int(R.bits(x)[0]) for x in M.levels(u(2))] == [1, 2, 4, 7] and [int(R.bits(x)[0]) for x in M.levels(u(3))] == [1, 3, 6, 10]
    # saturation: thresholds and levels at the four scales around 65504 / 3.375, / 2.625, / 1.5 and at 65504
    sc = u(0x74BD, 0x74BE, 0x7617, 0x7618, 0x7954, 0x7955, 0x7BFF)                          # 19408, 19424 | 24944, 24960 | 43648, 43680 | 65504
    th, lv = M.thresholds(sc), M.levels(sc)
    assert R.bits(lv[3]).tolist() == [0x7BFF] * 7 and float(lv[3][0]) == 65504.0            # 19408 x 3.375 = 65502: rounds to 65504, no clamp yet
    assert R.bits(th[2]).tolist() == [R.bits(F16(19408 * 2.625)), R.bits(F16(19424 * 2.625)), 0x7BFE, 0x7BFF, 0x7BFF, 0x7BFF, 0x7BFF]
    assert R.bits(th[1]).tolist()[4:] == [0x7BFE, 0x7BFF, 0x7BFF] and R.bits(th[0]).tolist()[6] == R.bits(F16(49120))       # 49128: ulp 32, a tie
    assert np.isfinite(np.stack(th + lv).astype(np.float64)).all()
    # a block of +-65504: s = 65504, every element above t_0 = 49120 only: mag 1, recv = +-min(73692, 65504)
    s, sg, mg, r = enc((np.where(np.arange(B) % 2, -1, 1) * 65504.0).astype(F16))
    assert s == 0x7BFF and (mg == 1).all() and set(r.tolist()) == {0x7BFF, 0xFBFF}
    # the fp32 conversion of the sum rounds first (bblock's corner): 2^24 + 2^13 + 1 units is a tie in fp32 and goes to the even side
    lo = F16(1.0 / B)
    v = z.copy()
    v[:3] = [1.0, np.ldexp(1.0, -11), u(1)[0]]
    assert enc(v)[0] == R.bits(lo)


def test_nothing_leaks_between_blocks():
    """a block of tiny values between blocks of huge ones, and the last block of a row against the first of the next: every scale is its
    own block's mean, and every level is a level of its own block's scale"""
    for N, C in ((3, 192), (5, 320), (129, 128)):
        for B in BK.blocks_of(N, C):
            x, _ = BK.build("neighbours", N, C, B, nobase=True)
            d = x.view(F16)
            pkt, recv = M.compress(d, None, B)
            s = M.split(pkt, N, C, B)[2].astype(np.float64).reshape(-1)
            a = np.abs(d.astype(np.float64)).reshape(-1, B)
            assert ((s >= a.min(axis=1)) & (s <= a.max(axis=1))).all()
            big = s > 1000
            assert big.any() and (~big).any() and (s[~big] < 1e-5).all() and (big[1:] != big[:-1]).all()
            r = np.abs(recv.astype(np.float64)).reshape(-1, B)
            assert (r[~big] < 1e-4).all() and (r[big] > 300).all()


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
    N, C, B = 5, 320, 64
    x, base = BK.build("random", N, C, B, bf16=True)
    pkt, _ = M.step(x, base, B, True)
    d16 = M.BC.delta(x, base)
    pkt16, recv = M.compress(d16, None, B)
    assert np.array_equal(pkt, pkt16)
    state16 = np.random.default_rng(1).standard_normal((N, C)).astype(F16)
    assert np.array_equal(R.bits(M.residual_decompress(pkt, state16, N, C, B)), R.bits((state16 + recv).astype(F16)))


def test_hi_section_and_scales_are_a_two_bit_packet_of_the_same_block_scale():
    """sign and scale sections are what INT2_BLOCK sends for the same deltas: the sign bit of every hi code and every scale, bit for bit"""
    N, C, B = 5, 320, 32
    x, base = BK.build("random", N, C, B)
    hi, _, s = M.split(M.step(x, base, B, False)[0], N, C, B)
    codes2, s2 = I2.split(I2.step(x, base, B, False)[0], N, C, B)
    assert np.array_equal(R.bits(s), R.bits(s2)) and np.array_equal(R.unpack_int2(hi) >> 1, R.unpack_int2(codes2) >> 1)


# ---- quality on the G12 drift --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _g12(seed):
    """the G12 inputs of one tensor (bits, 28 steps) and the MXFP4 contract's error per step on them (step 0 is the warm-up)"""
    spec = importlib.util.spec_from_file_location("make_golden_quality", os.path.join(REPO, "tests", "golden", "make_golden_quality.py"))
    mq = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mq)
    assert (mq.N, mq.C) == (128, 3072)
    xs = [R.bits(x.numpy()).reshape(mq.N, mq.C).copy() for x in mq.drift(seed, 28)]
    return xs, _trace(xs, lambda x, st: R.bits(MX.residual_compress(x.view(F16), st.view(F16))[1]))


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
def test_g12_error_between_int2_block_and_mxfp4(seed, B):
    """The contract's error-feedback trace on the G12 drift inputs ((128, 3072), 28 steps; K: seed 4242, V: 4243).  On EVERY step the
    error is strictly below INT2_BLOCK's contract at the same block size and at most 0.55 x it - a float model of the codec gave a worst
    per-step ratio of 0.525; the margin covers model against contract and nothing else - and above the MXFP4 contract's on the same inputs
    (a 3-bit code that beat 4.25 bits would mean the harness is wrong)."""
    xs, e_mx = _g12(seed)
    e_own = _trace(xs, lambda x, st: M.step(x, st, B, False)[1])
    e_i2 = _trace(xs, lambda x, st: I2.step(x, st, B, False)[1])
    ratio = e_own / e_i2
    print(f"seed {seed} B {B}: int3-block mean {e_own.mean():.4f} max {e_own.max():.4f}; int2-block mean {e_i2.mean():.4f}; "
          f"mxfp4 mean {e_mx.mean():.4f} max {e_mx.max():.4f}; ratio to int2-block min {ratio.min():.4f} max {ratio.max():.4f}; "
          f"least ratio to mxfp4 {(e_own / e_mx).min():.4f}")
    assert len(e_own) == 27
    assert (e_own < e_i2).all(), (e_own, e_i2)
    assert (ratio <= 0.55).all(), ratio.max()
    assert (e_own > e_mx).all(), (e_own, e_mx)
