"""The contract of the block-scaled 2-bit wire codec (include/cfx.h, CFX_CODEC_INT2_BLOCK = 12) in numpy - the statement the kernels are
held to, for fp16 and for bf16 activations.  B = param in {32, 64, 128}; a block is B consecutive elements of a row.

    d     = fp16(x - base)                      bf16: fp16_rne(fp32(x) - fp32(base))       base None: x
    s     = fp16( fp32(exact sum of |d| over the block, in units of 2^-24) / fp32(B) )      = oracle/ref_np.py mean16_exact
    code  = (d >= 0) << 1 | (|d| > s)           (-0 gives sign 1; the compare is strict)
    small = fp16(0.5 * s)    large = fp16(min(2 * fp32(s), 65504))
    recv  = (sign ? + : -) (mag ? large : small)
    new_base = recon = fp16(base + recv)        bf16: bf16_rne(fp32(base) + fp32(recv))    base None: recv;  no error feedback: x
    wire [ codes (N, C/4) bytes, INT2's code layout | scales (N, C/B) fp16 ]

fp16 tensors are fp16 arrays (or their uint16 bits), bf16 tensors uint16 bit patterns (tests/bf16_contract.py).  Plain helper module (no
tests here: tests/test_int2block_contract.py holds it to the witness of tests/_int2block_f64_check.py)."""
import numpy as np

import bf16_contract as BC
from oracle import ref_np as R

F16, F32 = np.float16, np.float32
NAME, CID = "int2-block", 12
BLOCKS = (32, 64, 128)
ELEM_BF16 = 0x100


def shape_ok(N, C, B):
    return B in BLOCKS and N >= 1 and C >= 1 and C % max(B, 64) == 0


def packet_bytes(N, C, B):
    return N * C // 4 + 2 * (N * C // B)


def packet_halves(N, C, B):
    return packet_bytes(N, C, B) // 2


def scales(d16, B):
    """(N, C) fp16 deltas -> (N, C/B) fp16 block scales"""
    N, C = d16.shape
    return R.mean16_exact(np.abs(d16).reshape(N, C // B, B), 2)


def codes_of(d16, s16, B):
    """fp16 deltas (N, C), scales (N, C/B) -> codes (N, C) in 0 .. 3"""
    thr = np.repeat(s16, B, axis=1)
    return (((d16 >= 0).astype(np.uint8) << 1) | (np.abs(d16) > thr).astype(np.uint8)).astype(np.uint8)


def levels(s16):
    """scales -> (small, large) fp16: INT2's 0.5 thr and 2 thr (R.int2_levels), the large one held to 65504"""
    small = (F16(0.5) * s16).astype(F16)
    large = np.minimum(F32(2.0) * s16.astype(F32), F32(65504.0)).astype(F16)
    return small, large


def recv_of(codes, s16, B):
    """codes (N, C), scales (N, C/B) -> recv fp16 (N, C): a level's bits with the sign bit of a cleared sign"""
    small, large = levels(s16)
    lvl = np.where((codes & 1) == 1, np.repeat(R.bits(large), B, axis=1), np.repeat(R.bits(small), B, axis=1)).astype(np.uint16)
    return (lvl | ((1 - (codes >> 1).astype(np.uint16)) << 15)).astype(np.uint16).view(F16)


def encode(d16, B):
    """fp16 deltas -> (packet words uint16, recv fp16 (N, C)); recv = decode(packet) exactly"""
    d16 = np.ascontiguousarray(R.as_f16(d16))
    N, C = d16.shape
    assert shape_ok(N, C, B), (N, C, B)
    s = scales(d16, B)
    packed = R.pack_int2(codes_of(d16, s, B))
    pkt = np.concatenate([packed.reshape(-1), R.bits(s).reshape(-1).view(np.uint8)]).view(np.uint16)
    assert pkt.size == packet_halves(N, C, B)
    return pkt, recv_of(R.unpack_int2(packed), s, B)


def split(packet, N, C, B):
    """packet words -> (code bytes (N, C/4) uint8, scales (N, C/B) fp16)"""
    w = np.ascontiguousarray(np.asarray(packet).view(np.uint16).reshape(-1))
    assert w.size == packet_halves(N, C, B), (w.size, packet_halves(N, C, B))
    by = w.view(np.uint8)
    return by[:N * C // 4].reshape(N, C // 4), by[N * C // 4:].view(F16).reshape(N, C // B)


def decode(packet, N, C, B):
    """packet words -> recv (N, C) fp16 (no base add)"""
    packed, s = split(packet, N, C, B)
    return recv_of(R.unpack_int2(packed), s, B)


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
