"""The bf16 form of the 1-bit and 2-bit exchange checked against its DEFINITION (include/cfx.h, "bf16 activations") without going through
tests/bf16_contract.py or the oracle - a helper next to tests/_f64_check.py, not a test.  bf16 tensors are uint16 bit patterns.

    check(name, x, base, packet_words, state)        a compress result: packet and error-feedback state
    check_state(name, base, packet_words, state)     a reconstruction alone (any packet, e.g. a hand-built one)

d: the float64 difference of the two bf16 values, rounded ONCE to fp16 (delta16).  d then goes to the float64 bounds of _f64_check.py
as the codec's input: scales within 1 (V, chan) and 4 (U, tok) fp16 ulp, sign bits == (d >= 0) exactly, 2-bit magnitude bits exact
against the packet's own scales.

State: state == bf16_rne(fp32(base) + fp32(decode(packet))) bit for bit (base None: bf16_rne(fp32(decode(packet))), which keeps the
sign of a zero).  This is the TWO-step definition of include/cfx.h - an fp32 sum, rounded to fp32, then one rounding to bf16 - and NOT a
single rounding of the exact sum: fp32(base) + fp32(recv) can need more than 24 bits, and the fp32 rounding can then land on a bf16 tie
the exact sum was not on.  The fp32 sum and the rounding to bf16 are torch's on the CPU (`.to(torch.bfloat16)`), a second implementation
beside bf16_contract.f32_to_bf16's integer arithmetic.  decode(packet) is the fp16 arithmetic the codec defines (fp16(U * V); fp16(chan *
tok) and its 0.5 / 2.0 levels), written out here from the wire layout."""
import numpy as np
import torch

import _f64_check as F

F16, F32, F64 = np.float16, np.float32, np.float64


def widen64(u16):
    """bf16 bits -> the exact value, float64"""
    return (np.ascontiguousarray(u16).astype(np.uint32) << 16).view(F32).astype(F64)


def delta16(x, base):
    """d = fp16(x - base), the difference taken exactly (float64) and rounded once.  The contract subtracts in fp32 first; that is the same
    value: a bf16 significand has 8 bits, so x - base is exact in fp32 unless the operands' exponents are 17 or more apart, and then the
    larger one (8 bits: an fp16 value, far from any fp16 tie) decides the rounding alone - except below 2^-14, where an 8-bit value can
    sit on a tie of fp16's subnormal grid; the value domain keeps such pairs within 2^16 of each other, and this function refuses a
    pair on which the two definitions differ rather than pick one."""
    x64 = widen64(x)
    d64 = x64 if base is None else x64 - widen64(base)
    assert np.isfinite(d64).all() and (np.abs(d64) < 65504).all(), "outside the documented domain: finite values, |x - base| < 65504"
    with np.errstate(over="ignore"):
        d = d64.astype(F16)
        two_step = d64.astype(F32).astype(F16)
    bad = d.view(np.uint16) != two_step.view(np.uint16)
    assert not bad.any(), f"{int(bad.sum())} pairs where fp16(fp32(x - base)) is not the single rounding: outside this check's domain"
    return d


def decode(name, pkt, N, C):
    """(recv fp16 (N, C), as the codec defines it from the packet's own bits and scales)"""
    per = {"binary": 8, "int2": 4}[name]
    codes, rs, cs = F._split(pkt, [N * C // per, 2 * N, 2 * C])
    rs, cs = rs.view(F16).reshape(-1, 1), cs.view(F16).reshape(1, -1)
    with np.errstate(over="ignore"):
        if name == "binary":
            sign = ((codes.reshape(N, C // 8)[:, :, None] >> np.arange(8, dtype=np.uint8)) & 1).reshape(N, C).astype(bool)
            mag = (rs * cs).astype(F16)                                                   # fp16(U[n] * V[c])
        else:
            idx = ((codes.reshape(N, C // 4)[:, :, None] >> (2 * np.arange(4, dtype=np.uint8))) & 3).reshape(N, C)
            sign = (idx >> 1).astype(bool)
            thr = (cs * rs).astype(F16)                                                   # fp16(chan[c] * tok[n])
            mag = np.where((idx & 1).astype(bool), (F16(2.0) * thr).astype(F16), (F16(0.5) * thr).astype(F16))
    return np.where(sign, mag, -mag).astype(F16)


def _torch_bf16(u16):
    return torch.from_numpy(np.ascontiguousarray(u16).view(np.int16).copy()).view(torch.bfloat16)


def state_of(base, recv16):
    """bf16_rne(fp32(base) + fp32(recv)) as torch computes it on the CPU: uint16 bits"""
    r = torch.from_numpy(np.ascontiguousarray(recv16)).to(torch.float32)
    s = r if base is None else _torch_bf16(base).to(torch.float32).reshape(r.shape) + r
    return s.to(torch.bfloat16).contiguous().view(torch.int16).numpy().view(np.uint16)


def check_state(name, base, pkt, state, N=None, C=None):
    if N is None:
        N, C = np.asarray(state).shape
    want = state_of(base, decode(name, pkt, N, C))
    got = np.asarray(state).view(np.uint16).reshape(N, C)
    bad = got != want
    assert not bad.any(), (f"{name}: {int(bad.sum())}/{bad.size} state elements differ from bf16(fp32(base) + fp32(decode(packet))) "
                           f"(first at {tuple(int(i) for i in np.argwhere(bad)[0])})")


def check(name, x, base, pkt, state=None):
    assert name in ("binary", "int2"), name
    d = delta16(x, base)
    F.check(name, 0, d, None, pkt, None)                  # the fp16 path's float64 bounds, on d
    if state is not None:
        check_state(name, base, pkt, state, *d.shape)
