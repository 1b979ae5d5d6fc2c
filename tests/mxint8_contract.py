"""The contract of the MXINT8 wire codec (include/cfx.h, CFX_CODEC_MXINT8 = 16) in numpy - the statement the kernels are held to, for fp16
and for bf16 activations, written from the bits: the shared exponent from the fp16 BITS of the block maximum, the element from the exact
fp32 product y = d * 2^(6-X).

    d = fp16(x - base)    bf16: fp16_rne(fp32(x) - fp32(base))    base None: x
    a = max over a block of 32 of (bits(d) & 0x7fff) ; a >= 0x7c00: scale byte 0xFF, codes 0, the block reconstructs to NaN (0x7e00)
    X = max(floor(log2 |d|max), -18) ; scale byte X + 127
    q = clamp(rne(d * 2^(6-X)), -127, 127) ; code = q as a two's-complement byte ; recv = q * 2^(X-6)   (byte 0x80 reads as -127)
    new_base = recon = fp16(base + recv)    bf16: bf16_rne(fp32(base) + fp32(recv))    base None: recv;  no error feedback: x
    wire [ codes (N, C) bytes | scale (N, C/32) bytes ]

fp16 tensors are fp16 arrays (or their uint16 bits), bf16 tensors uint16 bit patterns (tests/bf16_contract.py).  Plain helper module (no
tests here: tests/test_mxint8_contract.py holds it to the integer witness of tests/_mxint8_f64_check.py)."""
import numpy as np

import bf16_contract as BC
from oracle import ref_np as R

F16, F32 = np.float16, np.float32
NAME, CID, BLOCK = "mxint8", 16, 32
ELEM_BF16 = 0x100
NAN_BITS = np.uint16(0x7E00)
X_MIN = -18


def shape_ok(N, C):
    return N >= 1 and C >= 1 and C % 64 == 0


def packet_bytes(N, C):
    return N * C + N * C // 32


def packet_halves(N, C):
    return packet_bytes(N, C) // 2


def scale_bytes(d16):
    """(N, C) fp16 deltas -> (N, C/32) uint8 scale bytes, from the bits"""
    N, C = d16.shape
    a = (R.bits(d16).reshape(N, C // BLOCK, BLOCK) & 0x7FFF).max(axis=2).astype(np.int64)
    msb = np.zeros_like(a)
    for k in range(1, 10):                                  # index of the leading bit of a subnormal maximum (a < 0x400)
        msb[a >= (1 << k)] = k
    e = np.where(a >= 0x400, (a >> 10) - 15, msb - 24)
    e = np.maximum(e, X_MIN)
    return np.where(a >= 0x7C00, 0xFF, e + 127).astype(np.uint8)


def codes(d16, sb):
    """(N, C) fp16 deltas, (N, C/32) scale bytes -> (N, C) int8 codes"""
    s = np.repeat(sb, BLOCK, axis=1).astype(np.int64)
    ok = s != 0xFF
    inv = np.ldexp(F32(1), np.where(ok, 133 - s, 0).astype(np.int32)).astype(F32)            # 2^(6-X)
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.where(ok, R.as_f16(d16), F16(0)).astype(F32) * inv                           # exact: 11 bits times a power of two
    assert y.dtype == F32 and (np.abs(y) < 128).all()
    q = np.clip(np.rint(y), -127, 127).astype(np.int8)                                      # np.rint: to nearest, ties to even
    return q


def recv_of(q, sb):
    """codes (N, C) int8, scale bytes (N, C/32) -> recv fp16 (N, C): exact in fp16, +0 for q == 0; a 0xFF block is NaN"""
    s = np.repeat(sb, BLOCK, axis=1).astype(np.int32)
    ok = s != 0xFF
    qi = np.maximum(q.astype(np.int32), -127)
    v = np.ldexp(qi.astype(F32), np.where(ok, s - 133, 0)).astype(F32)
    h = v.astype(F16)
    assert np.array_equal(h.astype(F32)[ok], v[ok]), "decode leaves fp16"
    out = np.where(qi == 0, np.uint16(0), R.bits(h))
    return np.where(ok, out, NAN_BITS).astype(np.uint16).view(F16)


def encode(d16):
    """fp16 deltas -> (packet words uint16, recv fp16 (N, C)); recv = decode(packet) exactly"""
    d16 = np.ascontiguousarray(R.as_f16(d16))
    N, C = d16.shape
    assert shape_ok(N, C), (N, C)
    sb = scale_bytes(d16)
    q = codes(d16, sb)
    pkt = np.concatenate([q.reshape(-1).view(np.uint8), sb.reshape(-1)]).view(np.uint16)
    assert pkt.size == packet_halves(N, C)
    return pkt, recv_of(q, sb)


def split(packet, N, C):
    """packet words -> (codes (N, C) int8, scale bytes (N, C/32) uint8)"""
    w = np.ascontiguousarray(np.asarray(packet).view(np.uint16).reshape(-1))
    assert w.size == packet_halves(N, C), (w.size, packet_halves(N, C))
    by = w.view(np.uint8)
    return by[:N * C].view(np.int8).reshape(N, C), by[N * C:].reshape(N, C // BLOCK)


def decode(packet, N, C):
    """packet words -> recv (N, C) fp16 (no base add)"""
    return recv_of(*split(packet, N, C))


# ---- fp16 activations ---------------------------------------------------------------------------------------------------------------
def compress(x, base):
    """-> (packet, recv)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return encode(R._delta(x, base))


def decompress(packet, N, C):
    return decode(packet, N, C)


def residual_compress(x, base, ef=True):
    """(packet, new_base fp16)"""
    pkt, recv = compress(x, base)
    with np.errstate(invalid="ignore", over="ignore"):
        return pkt, (R._add_base(base, recv) if ef else R.as_f16(x).copy())


def residual_decompress(packet, base, N, C):
    with np.errstate(invalid="ignore", over="ignore"):
        return R._add_base(base, decode(packet, N, C))


# ---- bf16 activations (uint16 bit patterns) -------------------------------------------------------------------------------------------
def residual_compress_bf16(x_u16, base_u16, ef=True):
    """(packet, new_base bf16 bits)"""
    with np.errstate(invalid="ignore", over="ignore"):
        pkt, recv = encode(BC.delta(x_u16, base_u16))
        return pkt, (BC.add_base(base_u16, recv) if ef else np.array(x_u16, dtype=np.uint16, copy=True))


def residual_decompress_bf16(packet, base_u16, N, C):
    """recon bf16 bits"""
    with np.errstate(invalid="ignore", over="ignore"):
        return BC.add_base(base_u16, decode(packet, N, C))


def step(x_u16, base_u16, bf16, ef=True):
    """one residual compress on bit patterns of either element type -> (packet words, new state bits)"""
    if bf16:
        return residual_compress_bf16(x_u16, base_u16, ef)
    pkt, nb = residual_compress(np.asarray(x_u16).view(F16), None if base_u16 is None else np.asarray(base_u16).view(F16), ef)
    return pkt, R.bits(nb)


def recon(packet, base_u16, N, C, bf16):
    """a receiver's reconstruction on bit patterns of either element type -> state bits"""
    if bf16:
        return residual_decompress_bf16(packet, base_u16, N, C)
    return R.bits(residual_decompress(packet, None if base_u16 is None else np.asarray(base_u16).view(F16), N, C))
