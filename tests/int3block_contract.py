"""The contract of the block-scaled 3-bit wire codec (include/cfx.h, CFX_CODEC_INT3_BLOCK = 14) in numpy - the statement the kernels are
held to, for fp16 and for bf16 activations.  B = param in {32, 64, 128}; a block is B consecutive elements of a row.

    d     = fp16(x - base)                      bf16: fp16_rne(fp32(x) - fp32(base))       base None: x
    s     = fp16( fp32(exact sum of |d| over the block, in units of 2^-24) / fp32(B) )      = oracle/ref_np.py mean16_exact
    t_k   = fp16( min( fp32(s) * T_k, 65504 ) )       T = (0.75, 1.5, 2.625)
    l_k   = fp16( min( fp32(s) * L_k, 65504 ) )       L = (0.375, 1.125, 1.875, 3.375)
    sign  = d >= 0  (-0 gives 1)                mag = (|d| > t_0) + (|d| > t_1) + (|d| > t_2)      (strict)
    recv  = (sign ? + : -) l_mag
    new_base = recon = fp16(base + recv)        bf16: bf16_rne(fp32(base) + fp32(recv))    base None: recv;  no error feedback: x
    wire [ hi (N, C/4) bytes: sign << 1 | mag >> 1 in INT2's code layout | lo (N, C/8) bytes: mag & 1 in BINARY's bit layout |
           scales (N, C/B) fp16 ]

fp16 tensors are fp16 arrays (or their uint16 bits), bf16 tensors uint16 bit patterns (tests/bf16_contract.py).  Plain helper module (no
tests here: tests/test_int3block_contract.py holds it to the witness of tests/_int3block_f64_check.py)."""
import numpy as np

import bf16_contract as BC
from oracle import ref_np as R

F16, F32 = np.float16, np.float32
NAME, CID = "int3-block", 14
BLOCKS = (32, 64, 128)
ELEM_BF16 = 0x100
T = (0.75, 1.5, 2.625)
L = (0.375, 1.125, 1.875, 3.375)


def shape_ok(N, C, B):
    return B in BLOCKS and N >= 1 and C >= 1 and C % max(B, 64) == 0


def packet_bytes(N, C, B):
    return N * C // 4 + N * C // 8 + 2 * (N * C // B)


def packet_halves(N, C, B):
    return packet_bytes(N, C, B) // 2


def scales(d16, B):
    """(N, C) fp16 deltas -> (N, C/B) fp16 block scales"""
    N, C = d16.shape
    return R.mean16_exact(np.abs(d16).reshape(N, C // B, B), 2)


def scaled(s16, k):
    """fp16( min( fp32(s) * k, 65504 ) ): the product is exact in fp32, the conversion is numpy's - to nearest even, subnormals included"""
    return np.minimum(s16.astype(F32) * F32(k), F32(65504.0)).astype(F16)


def thresholds(s16):
    return tuple(scaled(s16, k) for k in T)


def levels(s16):
    return tuple(scaled(s16, k) for k in L)


def mags_of(d16, s16, B):
    """fp16 deltas (N, C), scales (N, C/B) -> mag (N, C) in 0 .. 3"""
    a = np.abs(d16)
    m = np.zeros(d16.shape, dtype=np.uint8)
    for t in thresholds(s16):
        m += (a > np.repeat(t, B, axis=1)).astype(np.uint8)
    return m


def recv_of(sign, mag, s16, B):
    """sign bits, mags (N, C), scales (N, C/B) -> recv fp16 (N, C): a level's bits with the sign bit of a cleared sign"""
    lv = np.stack([np.repeat(R.bits(l), B, axis=1) for l in levels(s16)])                      # (4, N, C)
    lvl = np.take_along_axis(lv, mag[None].astype(np.int64), axis=0)[0].astype(np.uint16)
    return (lvl | ((1 - sign.astype(np.uint16)) << 15)).astype(np.uint16).view(F16)


def pack(sign, mag):
    """-> (hi (N, C/4) uint8, lo (N, C/8) uint8)"""
    N, C = mag.shape
    hi = R.pack_int2(((sign.astype(np.uint8) << 1) | (mag >> 1)).astype(np.uint8))
    b = (mag & 1).astype(np.uint8).reshape(N, C // 8, 8)
    lo = (b << np.arange(8, dtype=np.uint8)).sum(axis=2).astype(np.uint8)
    return hi, lo


def unpack(hi, lo):
    """-> (sign, mag) (N, C) uint8"""
    c = R.unpack_int2(hi)
    return (c >> 1).astype(np.uint8), (((c & 1) << 1) | R.unpack_bits_1(lo)).astype(np.uint8)


def encode(d16, B):
    """fp16 deltas -> (packet words uint16, recv fp16 (N, C)); recv = decode(packet) exactly"""
    d16 = np.ascontiguousarray(R.as_f16(d16))
    N, C = d16.shape
    assert shape_ok(N, C, B), (N, C, B)
    s = scales(d16, B)
    sign, mag = (d16 >= 0).astype(np.uint8), mags_of(d16, s, B)
    hi, lo = pack(sign, mag)
    pkt = np.concatenate([hi.reshape(-1), lo.reshape(-1), R.bits(s).reshape(-1).view(np.uint8)]).view(np.uint16)
    assert pkt.size == packet_halves(N, C, B)
    return pkt, recv_of(sign, mag, s, B)


def split(packet, N, C, B):
    """packet words -> (hi bytes (N, C/4) uint8, lo bytes (N, C/8) uint8, scales (N, C/B) fp16)"""
    w = np.ascontiguousarray(np.asarray(packet).view(np.uint16).reshape(-1))
    assert w.size == packet_halves(N, C, B), (w.size, packet_halves(N, C, B))
    by = w.view(np.uint8)
    E = N * C
    return by[:E // 4].reshape(N, C // 4), by[E // 4:3 * E // 8].reshape(N, C // 8), by[3 * E // 8:].view(F16).reshape(N, C // B)


def decode(packet, N, C, B):
    """packet words -> recv (N, C) fp16 (no base add)"""
    hi, lo, s = split(packet, N, C, B)
    return recv_of(*unpack(hi, lo), s, B)


# ---- fp16 activations ---------------------------------------------------------------------------------------------------------------
def compress(x, base, B):
    """-> (packet, recv)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return encode(R._delta(x, base), B)


def decompress(packet, N, C, B):
    return decode(packet, N, C, B)


def residual_compress(x, base, B, ef=True):
    """(packet, new_base fp16)"""
    pkt, recv = compress(x, base, B)
    return pkt, (R._add_base(base, recv) if ef else R.as_f16(x).copy())


def residual_decompress(packet, base, N, C, B):
    return R._add_base(base, decode(packet, N, C, B))


# ---- bf16 activations (uint16 bit patterns) -------------------------------------------------------------------------------------------
def residual_compress_bf16(x_u16, base_u16, B, ef=True):
    """(packet, new_base bf16 bits)"""
    pkt, recv = encode(BC.delta(x_u16, base_u16), B)
    return pkt, (BC.add_base(base_u16, recv) if ef else np.array(x_u16, dtype=np.uint16, copy=True))


def residual_decompress_bf16(packet, base_u16, N, C, B):
    """recon bf16 bits"""
    return BC.add_base(base_u16, decode(packet, N, C, B))


def step(x_u16, base_u16, B, bf16, ef=True):
    """one residual compress on bit patterns of either element type -> (packet words, new state bits)"""
    if bf16:
        return residual_compress_bf16(x_u16, base_u16, B, ef)
    pkt, nb = residual_compress(np.asarray(x_u16).view(F16), None if base_u16 is None else np.asarray(base_u16).view(F16), B, ef)
    return pkt, R.bits(nb)


def recon(packet, base_u16, N, C, B, bf16):
    """a receiver's reconstruction on bit patterns of either element type -> state bits"""
    if bf16:
        return residual_decompress_bf16(packet, base_u16, N, C, B)
    return R.bits(residual_decompress(packet, None if base_u16 is None else np.asarray(base_u16).view(F16), N, C, B))
