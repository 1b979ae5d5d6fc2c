"""An independent witness of the block-scaled 1-bit codec (include/cfx.h, "BINARY_BLOCK"): it shares no code with
tests/bblock_contract.py.  Per block it adds the magnitudes as Python integers (units of 2^-24), rounds that integer ONCE to 24
significant bits - nearest, ties to even, in integer arithmetic: the fp32 conversion -, divides by B and rounds to fp16; the sign bits come
from the float64 deltas; the state is judged against the float64 sum of base and recv, rounded once (bf16: through fp32).

Bounds it derives, not measures: a mean lies between the block's smallest and largest magnitude, both fp16 values, and rounding is
monotone, so  min|d| <= s <= max|d| <= 65504  and, recv having d's sign,  |recv - d| <= max|d| - min|d|  over the block."""
import numpy as np

F16, F32, F64 = np.float16, np.float32, np.float64


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


def _u16(a):
    a = np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint16) if a.dtype != np.uint16 else a


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
    assert by.size == N * C // 8 + 2 * (N * C // B), "packet length"
    # ---- sign bits: bit i of byte j of row n says d[n, 8j+i] is not below zero (-0 is not)
    got_bits = ((by[:N * C // 8].reshape(N, C // 8, 1) >> np.arange(8)) & 1).reshape(N, C)
    want_bits = np.where(d < 0, 0, 1)
    bad = got_bits != want_bits
    assert not bad.any(), f"{int(bad.sum())} sign bits differ (first at {int(np.argmax(bad))})"
    # ---- scales: Python-integer block sums, one rounding to 24 bits, one to fp16
    units = np.rint(np.abs(d) * 16777216.0).astype(np.int64)
    assert np.array_equal(units.astype(F64) / 16777216.0, np.abs(d)), "a magnitude is not a whole number of 2^-24"
    blk = units.reshape(N * C // B, B)
    want_s = np.empty(N * C // B, dtype=F64)
    for i in range(blk.shape[0]):
        want_s[i] = float(_round24(sum(int(v) for v in blk[i]))) / 16777216.0 / B
    want_s16 = want_s.astype(F16)
    got_s16 = by[N * C // 8:].view(F16).reshape(-1)
    bad = got_s16.view(np.uint16) != want_s16.view(np.uint16)
    assert not bad.any(), (f"{int(bad.sum())} of {bad.size} block scales differ (first: block {int(np.argmax(bad))}, got "
                           f"{got_s16[bad][:1]}, want {want_s16[bad][:1]})")
    # ---- the derived bounds
    s = got_s16.astype(F64)
    a = np.abs(d).reshape(-1, B)
    assert (s >= a.min(axis=1)).all() and (s <= a.max(axis=1)).all() and (s <= 65504).all(), "a scale outside [min, max] of its block"
    recv = np.where(got_bits == 1, 1.0, -1.0) * np.repeat(s, B).reshape(N, C)
    assert (np.abs(recv - d).reshape(-1, B) <= (a.max(axis=1) - a.min(axis=1))[:, None]).all(), "recv further from d than the block's spread"
    if state is None:
        return
    st = _u16(state).reshape(N, C)
    if not ef:
        assert np.array_equal(st, xb), "state without error feedback is not x"
        return
    neg = (got_bits == 0)
    if bf16:
        want = _f32_to_bf16_bits((recv if b64 is None else b64 + recv).astype(F32))      # (-0.0 keeps its sign through both)
    elif b64 is None:
        want = (np.repeat(got_s16.view(np.uint16), B).reshape(N, C) | (neg.astype(np.uint16) << 15)).astype(np.uint16)
    else:
        want = np.ascontiguousarray((b64 + recv).astype(F16)).view(np.uint16)
    bad = st != want
    assert not bad.any(), f"state != round(base + recv): {int(bad.sum())} elements (first at {int(np.argmax(bad))})"
