"""The contract of the MXFP4 wire codec (include/cfx.h, CFX_CODEC_MXFP4 = 8) in numpy - the statement the kernels are held to, written
from the integer description: the shared exponent from the fp16 BITS of the block maximum, the element thresholds on the exact fp32
quotient y = |d| / 2^X.

    d = fp16(x - base) ; a = max over a block of 32 of (bits(d) & 0x7fff)
    a >= 0x7c00: scale byte 0xFF, codes 0, the block reconstructs to NaN
    e = max(floor(log2 |d|max), -21) ; X = e - 2 ; scale byte X + 127
    mag = nearest of {0, .5, 1, 1.5, 2, 3, 4, 6} to y, a tie to the even index, y > 6 -> 7 ; code = sign << 3 | mag
    recv = (+-) grid[mag] * 2^X ; wire [ codes (N, C/2) bytes, element 2j low nibble | scale (N, C/32) bytes ]

Plain helper module (no tests here: tests/test_mxfp4_contract.py holds it to the float64 witness of tests/_mxfp4_f64_check.py)."""
import numpy as np

from oracle import ref_np as R

F16, F32 = np.float16, np.float32
NAME, CID, BLOCK = "mxfp4", 8, 32
GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=F32)
NAN_BITS = np.uint16(0x7E00)


def packet_halves(N, C):
    return (N * C // 2 + N * C // 32) // 2


def scale_bytes(d16):
    """(N, C) fp16 deltas -> (N, C/32) uint8 scale bytes, from the bits"""
    N, C = d16.shape
    a = (R.bits(d16).reshape(N, C // BLOCK, BLOCK) & 0x7FFF).max(axis=2).astype(np.int64)
    msb = np.zeros_like(a)
    for k in range(1, 10):                                  # index of the leading bit of a subnormal maximum (a < 0x400)
        msb[a >= (1 << k)] = k
    e = np.where(a >= 0x400, (a >> 10) - 15, msb - 24)
    e = np.maximum(e, -21)
    return np.where(a >= 0x7C00, 0xFF, e - 2 + 127).astype(np.uint8)


def codes(d16, sb):
    """(N, C) fp16 deltas, (N, C/32) scale bytes -> (N, C) uint8 codes"""
    N, C = d16.shape
    b = R.bits(d16)
    s = np.repeat(sb, BLOCK, axis=1).astype(np.int64)
    ok = s != 0xFF
    inv = np.ldexp(F32(1), np.where(ok, 127 - s, 0).astype(np.int32)).astype(F32)            # 2^-X
    y = (b & 0x7FFF).view(F16).astype(F32) * inv                                            # exact: 11 bits times a power of two
    assert y.dtype == F32
    mag = ((y > F32(0.25)).astype(np.uint8) + (y >= F32(0.75)) + (y > F32(1.25)) + (y >= F32(1.75)) + (y > F32(2.5)) + (y >= F32(3.5))
           + (y > F32(5.0))).astype(np.uint8)
    c = (((b >> 15) << 3).astype(np.uint8) | mag).astype(np.uint8)
    return np.where(ok, c, 0).astype(np.uint8)


def pack(c):
    N, C = c.shape
    return (c[:, 0::2] | (c[:, 1::2] << 4)).astype(np.uint8)


def unpack(packed):
    N, C2 = packed.shape
    out = np.empty((N, C2 * 2), dtype=np.uint8)
    out[:, 0::2] = packed & 15
    out[:, 1::2] = packed >> 4
    return out


def recv_of(c, sb):
    """codes (N, C), scale bytes (N, C/32) -> recv fp16 (N, C): exact in fp16; a 0xFF block is NaN"""
    s = np.repeat(sb, BLOCK, axis=1).astype(np.int32)
    ok = s != 0xFF
    v = np.ldexp(GRID[c & 7], np.where(ok, s - 127, 0)).astype(F32)
    h = v.astype(F16)
    assert np.array_equal(h.astype(F32)[ok], v[ok]), "decode leaves fp16"
    out = R.bits(h) | ((c.astype(np.uint16) & 8) << 12)
    return np.where(ok, out, NAN_BITS).astype(np.uint16).view(F16)


def compress(x, base):
    """-> (packet words uint16, recv fp16 (N, C)); recv = decompress(packet) exactly"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.ascontiguousarray(R._delta(x, base))
    N, C = d.shape
    assert C % 64 == 0 and N >= 1
    sb = scale_bytes(d)
    c = codes(d, sb)
    pkt = np.concatenate([pack(c).reshape(-1), sb.reshape(-1)]).view(np.uint16)
    assert pkt.size == packet_halves(N, C)
    return pkt, recv_of(c, sb)


def split(packet, N, C):
    """packet words -> (codes (N, C) uint8, scale bytes (N, C/32) uint8)"""
    w = np.ascontiguousarray(np.asarray(packet).view(np.uint16).reshape(-1))
    assert w.size == packet_halves(N, C), (w.size, packet_halves(N, C))
    by = w.view(np.uint8)
    return unpack(by[:N * C // 2].reshape(N, C // 2)), by[N * C // 2:].reshape(N, C // BLOCK)


def decompress(packet, N, C):
    """packet words -> recv (N, C) fp16 (no base add)"""
    return recv_of(*split(packet, N, C))


def residual_compress(x, base, ef=True):
    """(packet, new_base) as R.residual_compress"""
    pkt, recv = compress(x, base)
    return pkt, (R._add_base(base, recv) if ef else R.as_f16(x).copy())


def residual_decompress(packet, base, N, C):
    return R._add_base(base, decompress(packet, N, C))
