"""The contract of the block-scaled 1-bit wire codec (include/cfx.h, CFX_CODEC_BINARY_BLOCK = 10) in numpy - the statement the kernels
are held to, for fp16 and for bf16 activations.  B = param in {32, 64, 128}; a block is B consecutive elements of a row.

    d    = fp16(x - base)                       bf16: fp16_rne(fp32(x) - fp32(base))       base None: x
    bit  = d >= 0                               (-0 gives 1; a NaN would give 0)
    s    = fp16( fp32(exact sum of |d| over the block, in units of 2^-24) / fp32(B) )       = oracle/ref_np.py mean16_exact
    recv = bit ? s : -s
    new_base = recon = fp16(base + recv)        bf16: bf16_rne(fp32(base) + fp32(recv))    base None: recv;  no error feedback: x
    wire [ bits (N, C/8) bytes, BINARY's bit layout | scales (N, C/B) fp16 ]

fp16 tensors are fp16 arrays (or their uint16 bits), bf16 tensors uint16 bit patterns (tests/bf16_contract.py).  Plain helper module (no
tests here: tests/test_bblock_contract.py holds it to the witness of tests/_bblock_f64_check.py)."""
import numpy as np

import bf16_contract as BC
from oracle import ref_np as R

F16 = np.float16
NAME, CID = "binary-block", 10
BLOCKS = (32, 64, 128)
ELEM_BF16 = 0x100


def shape_ok(N, C, B):
    return B in BLOCKS and N >= 1 and C >= 1 and C % max(B, 64) == 0


def packet_bytes(N, C, B):
    return N * C // 8 + 2 * (N * C // B)


def packet_halves(N, C, B):
    return packet_bytes(N, C, B) // 2


def scales(d16, B):
    """(N, C) fp16 deltas -> (N, C/B) fp16 block scales"""
    N, C = d16.shape
    return R.mean16_exact(np.abs(d16).reshape(N, C // B, B), 2)


def recv_of(bits01, s16, B):
    """sign bits (N, C) in {0, 1}, scales (N, C/B) -> recv fp16 (N, C): the scale's bits with the sign bit of a cleared bit"""
    sb = np.repeat(R.bits(s16), B, axis=1)
    return (sb | ((1 - bits01.astype(np.uint16)) << 15)).astype(np.uint16).view(F16)


def encode(d16, B):
    """fp16 deltas -> (packet words uint16, recv fp16 (N, C)); recv = decode(packet) exactly"""
    d16 = np.ascontiguousarray(R.as_f16(d16))
    N, C = d16.shape
    assert shape_ok(N, C, B), (N, C, B)
    packed, s = R.pack_bits_1(d16), scales(d16, B)
    pkt = np.concatenate([packed.reshape(-1), R.bits(s).reshape(-1).view(np.uint8)]).view(np.uint16)
    assert pkt.size == packet_halves(N, C, B)
    return pkt, recv_of(R.unpack_bits_1(packed), s, B)


def split(packet, N, C, B):
    """packet words -> (sign bytes (N, C/8) uint8, scales (N, C/B) fp16)"""
    w = np.ascontiguousarray(np.asarray(packet).view(np.uint16).reshape(-1))
    assert w.size == packet_halves(N, C, B), (w.size, packet_halves(N, C, B))
    by = w.view(np.uint8)
    return by[:N * C // 8].reshape(N, C // 8), by[N * C // 8:].view(F16).reshape(N, C // B)


def decode(packet, N, C, B):
    """packet words -> recv (N, C) fp16 (no base add)"""
    packed, s = split(packet, N, C, B)
    return recv_of(R.unpack_bits_1(packed), s, B)


# ---- fp16 activations ---------------------------------------------------------------------------------------------------------------
def compress(x, base, B):
    """-> (packet, recv)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return encode(R._delta(x, base), B)


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
