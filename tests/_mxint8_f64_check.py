"""An independent witness of the MXINT8 codec (include/cfx.h, "MXINT8"): it shares no code with tests/mxint8_contract.py and does the
codec's arithmetic on integers only.  |d| is taken in whole units of 2^-24 (every finite fp16 value is one); a block's X comes from the bit
length of its largest magnitude, X = max(bit_length - 25, -18); with sh = X + 18 >= 0 the element is q = the round-half-even shift of the
units by sh, held to 127, sent with d's sign (0 for q == 0), and a receiver adds q << sh units - an integer below 2^40 with at most 7
significant bits, so an fp16 value (asserted).  A block with a NaN or an inf delta must be the 0xFF block: codes 0, NaN states.  The
subtraction that makes d and the state are judged against float64, rounded once (bf16: through fp32), as tests/_bblock_f64_check.py does.

What it derives, not measures: sh == 0 (|d|max < 2^-17) reproduces the block exactly; |units - recv| <= 2^(sh-1) unless the element
saturates, and then it is below 2^sh; recv never has the sign opposite to d's."""
import numpy as np

F16, F32, F64 = np.float16, np.float32, np.float64
B = 32


def _bf16_to_f64(u16):
    return (np.asarray(u16).astype(np.uint32) * np.uint32(65536)).view(F32).astype(F64)


def _f32_to_bf16_bits(f32):
    """nearest, ties to even, finite values: on the integer bits"""
    u = np.ascontiguousarray(f32, dtype=F32).view(np.uint32).astype(np.uint64)
    low, keep = u & 0xFFFF, u >> 16
    up = (low > 0x8000) | ((low == 0x8000) & ((keep & 1) == 1))
    return (keep + up).astype(np.uint16)


def _u16(a):
    a = np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint16) if a.dtype != np.uint16 else a


def _units_of_bits(b):
    """fp16 bits of finite values -> whole units of 2^-24 of the magnitude (int64)"""
    b = b.astype(np.int64)
    e, m = (b >> 10) & 31, b & 1023
    return np.where(e > 0, (m | 1024) << np.maximum(e - 1, 0), m)


def _bits_of_units(r):
    """whole units of 2^-24 (int64, an fp16 value each: asserted) -> fp16 magnitude bits"""
    out = np.zeros(r.shape, dtype=np.int64)
    for i, v in enumerate(r.reshape(-1).tolist()):
        n = v.bit_length()
        if n <= 10:
            bits = v
        else:
            drop = n - 11
            assert v & ((1 << drop) - 1) == 0 and drop + 1 <= 30, "recv is no fp16 value"
            bits = ((drop + 1) << 10) | ((v >> drop) & 1023)
        out.reshape(-1)[i] = bits
    return out.astype(np.uint16)


def check(x, base, pkt, state=None, ef=True, bf16=False):
    """x, base: fp16 arrays or uint16 bit patterns (bf16: bit patterns); pkt: packet words; state: the sender's new state (bits)"""
    xb = _u16(x)
    N, C = xb.shape
    assert C % 64 == 0
    E, NB = N * C, N * C // B
    with np.errstate(over="ignore", invalid="ignore"):
        if bf16:
            x64 = _bf16_to_f64(xb)
            b64 = None if base is None else _bf16_to_f64(_u16(base))
            d16 = (x64 if b64 is None else x64 - b64).astype(F32).astype(F16)      # one fp32 rounding, one fp16 rounding
        else:
            x64 = xb.view(F16).astype(F64)
            b64 = None if base is None else _u16(base).view(F16).astype(F64)
            d16 = xb.view(F16).copy() if b64 is None else (x64 - b64).astype(F16)      # the correctly rounded difference
    db = np.ascontiguousarray(d16).view(np.uint16).reshape(NB, B)
    by = np.ascontiguousarray(np.asarray(pkt).view(np.uint16).reshape(-1)).view(np.uint8)
    assert by.size == E + E // B, "packet length"
    got_q = by[:E].view(np.int8).astype(np.int64).reshape(NB, B)
    got_s = by[E:].astype(np.int64)
    finite = ((db & 0x7FFF) < 0x7C00).all(axis=1)
    # ---- the 0xFF block
    assert np.array_equal(got_s == 0xFF, ~finite), "0xFF scale bytes are not exactly the blocks with a NaN or an inf"
    assert (got_q[~finite] == 0).all(), "a 0xFF block with a code byte that is not 0"
    # ---- finite blocks, on integers
    units = _units_of_bits(np.where(finite[:, None], db & 0x7FFF, 0))
    neg = (db >> 15).astype(np.int64)
    want_X = np.array([max(int(m).bit_length() - 25, -18) for m in units.max(axis=1)], dtype=np.int64)
    bad = finite & (got_s != want_X + 127)
    assert not bad.any(), f"{int(bad.sum())} of {NB} scale bytes differ (first: block {int(np.argmax(bad))}, got {got_s[bad][:1]}, want {(want_X + 127)[bad][:1]})"
    assert ((want_X >= -18) & (want_X <= 15)).all()
    sh = (want_X + 18)[:, None]
    q = units >> sh
    rem = units - (q << sh)
    half = np.where(sh > 0, np.int64(1) << np.maximum(sh - 1, 0), 0)
    q = q + ((sh > 0) & ((rem > half) | ((rem == half) & ((q & 1) == 1))))
    assert (q <= 128).all(), "y past 128"
    sat = q > 127
    q = np.minimum(q, 127)
    want_q = np.where(neg == 1, -q, q)
    bad = finite[:, None] & (got_q != want_q)
    assert not bad.any(), f"{int(bad.sum())} codes differ (first at {int(np.argmax(bad))}: got {got_q[bad][:1]}, want {want_q[bad][:1]})"
    assert (got_q != -128).all(), "-128 was sent"
    r = q << sh
    # ---- the derived bounds
    err = np.abs(units - r)
    assert (err[~sat] <= np.broadcast_to(half, err.shape)[~sat]).all(), "an unsaturated element further than half a step"
    assert (err[sat] < np.broadcast_to(np.int64(1) << sh, err.shape)[sat]).all(), "a saturated element a whole step away"
    assert (err[(sh == 0)[:, 0]] == 0).all(), "a block below 2^-17 is not exact"
    if state is None:
        return
    st = _u16(state).reshape(N, C)
    if not ef:
        assert np.array_equal(st, xb), "state without error feedback is not x"
        return
    fin = np.repeat(finite, B).reshape(N, C)
    recv_bits = (_bits_of_units(r) | np.where(q > 0, neg, 0).astype(np.uint16) << 15).astype(np.uint16).reshape(N, C)
    recv = recv_bits.view(F16).astype(F64)
    with np.errstate(over="ignore", invalid="ignore"):
        if bf16:
            want = _f32_to_bf16_bits((recv if b64 is None else b64 + recv).astype(F32))
        elif b64 is None:
            want = recv_bits
        else:
            want = np.ascontiguousarray((b64 + recv).astype(F16)).view(np.uint16)      # (a state past 65504 is inf on both sides)
    bad = fin & (st != want)
    assert not bad.any(), f"state != round(base + recv): {int(bad.sum())} elements (first at {int(np.argmax(bad))})"
    # a 0xFF block: every state is a NaN (no base, fp16: the bits 0x7e00)
    nan_st = (st & 0x7F80) == 0x7F80 if bf16 else (st & 0x7C00) == 0x7C00
    nan_st = nan_st & ((st & (0x7F if bf16 else 0x3FF)) != 0)
    assert nan_st[~fin].all(), "a state of a 0xFF block that is no NaN"
    if not bf16 and b64 is None:
        assert (st[~fin] == 0x7E00).all()
