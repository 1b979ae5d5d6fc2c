"""An independent witness of the block-scaled 3-bit codec (include/cfx.h, "INT3_BLOCK"): it shares no code with
tests/int3block_contract.py.  Per block it adds the magnitudes as Python integers (units of 2^-24), rounds that integer ONCE to 24
significant bits - nearest, ties to even, in integer arithmetic: the fp32 conversion -, divides by B as an exact rational and rounds that to
fp16 in integer arithmetic.  The three thresholds and the four levels are the exact rationals s * k (k in eighths: the product has at most
16 significant bits, so the fp32 product the contract names is this rational - asserted), held to 65504 and rounded to fp16 by the same
integer rounding; the magnitude compares whole units; the state is judged against the float64 sum of base and recv, rounded once (bf16:
through fp32).

What it derives, not measures: a mean lies between the block's smallest and largest magnitude, so  s <= 65504;  every |recv| is finite and
at most 65504; thresholds and levels do not decrease with k; an element sent at a higher magnitude is not smaller than one sent at a lower;
recv never has the sign opposite to d's."""
from fractions import Fraction

import numpy as np

F16, F32, F64 = np.float16, np.float32, np.float64
UNIT = Fraction(1, 1 << 24)


def _bf16_to_f64(u16):
    return (np.asarray(u16).astype(np.uint32) * np.uint32(65536)).view(F32).astype(F64)


def _f32_to_bf16_bits(f32):
    """nearest, ties to even, finite values: on the integer bits"""
    u = np.ascontiguousarray(f32, dtype=F32).view(np.uint32).astype(np.uint64)
    low, keep = u & 0xFFFF, u >> 16
    up = (low > 0x8000) | ((low == 0x8000) & ((keep & 1) == 1))
    return (keep + up).astype(np.uint16)


def _round24(s):
    """a non-negative Python integer to 24 significant bits, nearest, ties to even"""
    n = s.bit_length()
    if n <= 24:
        return s
    sh = n - 24
    q, rem, half = s >> sh, s & ((1 << sh) - 1), 1 << (sh - 1)
    if rem > half or (rem == half and (q & 1)):
        q += 1
    return q << sh


def _rne(fr):
    """a non-negative Fraction to the nearest integer, ties to even"""
    q, r = divmod(fr.numerator, fr.denominator)
    if 2 * r > fr.denominator or (2 * r == fr.denominator and (q & 1)):
        q += 1
    return q


def f16_bits_of(fr):
    """a non-negative Fraction (below 65520) to fp16 bits: nearest, ties to even, subnormals included - integer arithmetic only"""
    assert fr >= 0
    if fr == 0:
        return 0
    e = fr.numerator.bit_length() - fr.denominator.bit_length()
    if Fraction(2) ** e > fr:
        e -= 1
    assert Fraction(2) ** e <= fr < Fraction(2) ** (e + 1)
    e = max(e, -14)                              # the binade of fr, not below the subnormals' 2^-14
    n = _rne(fr / Fraction(2) ** (e - 10))       # in units of the binade's spacing: below 1024 subnormal, 2048: the next binade
    if n == 2048:
        n, e = 1024, e + 1
    assert e <= 15, "past fp16"
    return n if n < 1024 else ((e + 15) << 10) | (n - 1024)


def units_of_f16_bits(b):
    """fp16 bits of a finite non-negative value -> whole units of 2^-24"""
    e, m = (b >> 10) & 31, b & 1023
    assert e < 31
    return (m | 1024) << (e - 1) if e else m


def _u16(a):
    a = np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint16) if a.dtype != np.uint16 else a


T8 = (6, 12, 21)                # the thresholds 0.75, 1.5, 2.625 in eighths
L8 = (3, 9, 15, 27)             # the levels 0.375, 1.125, 1.875, 3.375 in eighths


def _scaled_bits(s_units, k8):
    """fp16 bits of min(s * k8 / 8, 65504), s in whole units of 2^-24: the product is an integer of at most 24 significant bits once its
    trailing zeros are dropped - what fp32 holds exactly - and is rounded once, to fp16"""
    p = s_units * k8
    assert p == 0 or (p >> ((p & -p).bit_length() - 1)).bit_length() <= 24, "the product is not an fp32 value"
    return f16_bits_of(min(Fraction(p, 8) * UNIT, Fraction(65504)))


def check(x, base, pkt, B, state=None, ef=True, bf16=False):
    """x, base: fp16 arrays or uint16 bit patterns (bf16: bit patterns); pkt: packet words; state: the sender's new state (bits)"""
    xb = _u16(x)
    N, C = xb.shape
    assert B in (32, 64, 128) and C % max(B, 64) == 0
    if bf16:
        x64 = _bf16_to_f64(xb)
        b64 = None if base is None else _bf16_to_f64(_u16(base))
        with np.errstate(over="ignore"):
            d16 = (x64 if b64 is None else x64 - b64).astype(F32).astype(F16)      # one fp32 rounding, one fp16 rounding
    else:
        x64 = xb.view(F16).astype(F64)
        b64 = None if base is None else _u16(base).view(F16).astype(F64)
        d16 = xb.view(F16).copy() if b64 is None else (x64 - b64).astype(F16)      # the correctly rounded difference
    d = d16.astype(F64)
    assert np.isfinite(d).all(), "outside the codec's domain"
    by = np.ascontiguousarray(np.asarray(pkt).view(np.uint16).reshape(-1)).view(np.uint8)
    E = N * C
    assert by.size == E // 4 + E // 8 + 2 * (E // B), "packet length"
    hi = ((by[:E // 4].reshape(N, C // 4, 1) >> (2 * np.arange(4))) & 3).reshape(N, C)
    lo = ((by[E // 4:E // 4 + E // 8].reshape(N, C // 8, 1) >> np.arange(8)) & 1).reshape(N, C)
    got_sign, got_mag = hi >> 1, ((hi & 1) << 1) | lo
    # ---- sign bits: d is not below zero (-0 is not)
    bad = got_sign != np.where(d < 0, 0, 1)
    assert not bad.any(), f"{int(bad.sum())} sign bits differ (first at {int(np.argmax(bad))})"
    # ---- scales: Python-integer block sums, one rounding to 24 bits, the exact quotient rounded to fp16
    units = np.rint(np.abs(d) * 16777216.0).astype(np.int64)
    assert np.array_equal(units.astype(F64) / 16777216.0, np.abs(d)), "a magnitude is not a whole number of 2^-24"
    blk = units.reshape(E // B, B)
    got_s = by[E // 4 + E // 8:].view(np.uint16).reshape(-1)
    want_s = np.array([f16_bits_of(_round24(sum(int(v) for v in row)) * UNIT / B) for row in blk], dtype=np.uint16)
    bad = got_s != want_s
    assert not bad.any(), (f"{int(bad.sum())} of {bad.size} block scales differ (first: block {int(np.argmax(bad))}, got "
                           f"{got_s[bad][:1]}, want {want_s[bad][:1]})")
    assert (got_s <= 0x7BFF).all(), "a scale past 65504"
    # ---- thresholds and levels from exact rationals: s * k in eighths, held to 65504, one rounding to fp16
    s_units = [units_of_f16_bits(int(b)) for b in got_s]
    thr = np.array([[units_of_f16_bits(_scaled_bits(u, k)) for k in T8] for u in s_units], dtype=np.int64)          # (blocks, 3) whole units
    lvl4 = np.array([[_scaled_bits(u, k) for k in L8] for u in s_units], dtype=np.uint16)                            # (blocks, 4) fp16 bits
    assert (np.diff(thr, axis=1) >= 0).all() and (np.diff(lvl4.astype(np.int64), axis=1) >= 0).all() and (lvl4 <= 0x7BFF).all()
    # ---- magnitudes: how many thresholds |d| exceeds, strictly, on whole units
    want_mag = (blk[:, :, None] > thr[:, None, :]).sum(axis=2)
    bad = got_mag.reshape(-1, B) != want_mag
    assert not bad.any(), f"{int(bad.sum())} magnitudes differ (first at {int(np.argmax(bad))})"
    lvl = np.take_along_axis(lvl4, got_mag.reshape(-1, B).astype(np.int64), axis=1).astype(np.uint16).reshape(N, C)
    recv_bits = (lvl | ((1 - got_sign).astype(np.uint16) << 15)).astype(np.uint16)
    recv = recv_bits.view(F16).astype(F64)
    assert np.isfinite(recv).all() and (np.abs(recv) <= 65504).all() and (recv * d >= 0).all(), "a level of the wrong sign or past 65504"
    if state is None:
        return
    st = _u16(state).reshape(N, C)
    if not ef:
        assert np.array_equal(st, xb), "state without error feedback is not x"
        return
    if bf16:
        want = _f32_to_bf16_bits((recv if b64 is None else b64 + recv).astype(F32))      # (-0.0 keeps its sign through both)
    elif b64 is None:
        want = recv_bits
    else:
        with np.errstate(over="ignore"):                         # (a state past 65504 is inf on both sides: outside the domain, still compared)
            want = np.ascontiguousarray((b64 + recv).astype(F16)).view(np.uint16)
    bad = st != want
    assert not bad.any(), f"state != round(base + recv): {int(bad.sum())} elements (first at {int(np.argmax(bad))})"
