"""Stand-alone quantisers - mirror of `xfuser/compact/compress_quantize.py` (quantize_1bit :7-90, dequantize_1bit
:154-225, quantize_int8/dequantize_int8 :428-484, quantize_int4/dequantize_int4 :522-640, quantize_int2/
dequantize_int2 :642-753, sim_binary :300-335, sim_int2 :338-384, sim_int4 :487-520), same signatures and returns.

All of them are the residual-0 (`base = NULL`) entry of the gfx950 kernels; returned parts are views into the packet.
Numerics follow the reference's EAGER semantics (fp16 rounding after every op); `@torch.compile`d reference code
differs from its own eager run and is matched to the reference's test tolerances only."""
from __future__ import annotations

import torch

from .. import codecs

K = codecs.Codec


def _nc(x):
    assert x.dtype == torch.half, "Input tensor must be FP16"
    assert x.dim() == 2, "Input tensor must be 2D"
    return x.contiguous()


def _cat_packet(*parts):
    return torch.cat([p.contiguous().view(-1).view(torch.half) if p.dtype != torch.half else p.reshape(-1) for p in parts])


# ---- 1 bit -------------------------------------------------------------------------------------------------------
def quantize_1bit(input_tensor: torch.Tensor, rank):
    """-> packed (N, C//8) uint8, scale_u (N,K), scale_v (K,C)   (rank = -1: K = 1 mean scales; rank 1..32: rank-K factors of |x|,
    compress_quantize.py:37-49 - note V is (K, C) here and (C, K) in the fastpath wire)."""
    assert rank >= 1 or rank == -1, "Rank must be >= 1 or -1"
    x = _nc(input_tensor)
    N, C = x.shape
    assert C % 8 == 0, "Channel dimension C must be divisible by 8 for packing"
    if rank != -1:
        from . import lowrank
        pkt = torch.empty(codecs.binary_rank_packet_halves(N, C, rank), dtype=torch.float16, device=x.device)
        codecs.binary_rank_compress_batch([x], [None], [None], [pkt], [lowrank._start(C, rank, x.device)], N, C, rank, update_cache=False)
        qh = N * C // 16
        return (pkt[:qh].view(torch.uint8).view(N, C // 8), pkt[qh:qh + N * rank].view(N, rank),
                pkt[qh + N * rank:].view(C, rank).t().contiguous())
    pkt, _ = codecs.compress(K.BINARY, x, None, N, C, update_cache=False)
    qh = N * C // 16
    return pkt[:qh].view(torch.uint8).view(N, C // 8), pkt[qh:qh + N].view(N, 1), pkt[qh + N:].view(1, C)


def dequantize_1bit(packed_tensor: torch.Tensor, scale_u: torch.Tensor, scale_v: torch.Tensor):
    assert packed_tensor.dtype == torch.uint8 and scale_u.dtype == torch.half and scale_v.dtype == torch.half
    N, C8 = packed_tensor.shape
    C = C8 * 8
    Kr = scale_u.shape[1]
    assert scale_u.shape == (N, Kr) and scale_v.shape == (Kr, C)
    if Kr > 1:
        out = torch.empty((N, C), dtype=torch.float16, device=packed_tensor.device)
        codecs.binary_rank_decompress_batch([_cat_packet(packed_tensor, scale_u, scale_v.t().contiguous())], [None], [out], N, C, Kr)
        return out
    return codecs.decompress(K.BINARY, _cat_packet(packed_tensor, scale_u, scale_v), None, N, C)


def sim_binary(input_tensor: torch.Tensor, rank=None):
    assert rank is not None, "Rank must be provided"
    x = _nc(input_tensor)
    return dequantize_1bit(*quantize_1bit(x, rank))


# ---- 2 bit -------------------------------------------------------------------------------------------------------
def quantize_int2(input_tensor: torch.Tensor):
    """-> packed (N, C//4) uint8, chan_scale (1,C), tok_scale (N,1)."""
    x = _nc(input_tensor)
    N, C = x.shape
    assert C % 4 == 0, f"Dimension C must be divisible by 4 for INT2 packing, got {C}"
    pkt, _ = codecs.compress(K.INT2, x, None, N, C, update_cache=False)
    qh = N * C // 8
    return pkt[:qh].view(torch.uint8).view(N, C // 4), pkt[qh + N:].view(1, C), pkt[qh:qh + N].view(N, 1)


def dequantize_int2(packed_indices: torch.Tensor, chan_scale: torch.Tensor, tok_scale: torch.Tensor):
    assert packed_indices.dtype == torch.uint8 and chan_scale.dtype == torch.half and tok_scale.dtype == torch.half
    N, C4 = packed_indices.shape
    C = C4 * 4
    assert chan_scale.shape == (1, C) and tok_scale.shape == (N, 1)
    return codecs.decompress(K.INT2, _cat_packet(packed_indices, tok_scale, chan_scale), None, N, C)


def sim_int2(input_tensor: torch.Tensor):
    return dequantize_int2(*quantize_int2(input_tensor))


def sim_int2_minmax(input_tensor: torch.Tensor):
    """4-level per-channel min/max quantise-dequantise (compress_quantize.py:386-426).  Simulation-only in the reference
    (quality studies), so this is plain tensor arithmetic on whatever device the input lives on, not a kernel."""
    x = _nc(input_tensor)
    lo = x.amin(dim=0, keepdim=True)
    step = ((x.amax(dim=0, keepdim=True) - lo) / (3 + 1e-6)).to(x.dtype)
    level = torch.clamp(torch.round((x - lo) / step), 0, 3).to(x.dtype)
    return level * step + lo


# ---- int8 --------------------------------------------------------------------------------------------------------
def quantize_int8(input_tensor: torch.Tensor):
    """-> q int8 (N,C), scale fp16 (1,C), zero_point int16 (1,C)."""
    x = _nc(input_tensor)
    N, C = x.shape
    pkt, _ = codecs.compress(K.INT8, x, None, N, C, update_cache=False)
    qh = N * C // 2
    return pkt[:qh].view(torch.int8).view(N, C), pkt[qh:qh + C].view(1, C), pkt[qh + C:].view(torch.int16).view(1, C)


def dequantize_int8(q_tensor, scale, zero_point):
    N, C = q_tensor.shape
    pkt = _cat_packet(q_tensor.view(torch.uint8), scale.reshape(-1), zero_point.reshape(-1).view(torch.half))
    return codecs.decompress(K.INT8, pkt, None, N, C)


# ---- int4 --------------------------------------------------------------------------------------------------------
def quantize_int4(input_tensor: torch.Tensor):
    """-> packed (N/2, C) uint8 [low nibble = even row], scale (1,C), min (1,C)."""
    x = _nc(input_tensor)
    N, C = x.shape
    assert N % 2 == 0, f"Dimension N (0) size must be even for INT4 packing, got {N}"
    pkt, _ = codecs.compress(K.INT4, x, None, N, C, update_cache=False)
    qh = N * C // 4
    return pkt[:qh].view(torch.uint8).view(N // 2, C), pkt[qh:qh + C].view(1, C), pkt[qh + C:].view(1, C)


def dequantize_int4(packed_tensor: torch.Tensor, scale: torch.Tensor, min_val: torch.Tensor):
    assert packed_tensor.dtype == torch.uint8 and scale.dtype == torch.half and min_val.dtype == torch.half
    N2, C = packed_tensor.shape
    return codecs.decompress(K.INT4, _cat_packet(packed_tensor, scale, min_val), None, N2 * 2, C)


# ---- 4-level min/max (extension: the reference only simulates it, sim_int2_minmax above) ---------------------------
def quantize_int2_minmax(input_tensor: torch.Tensor):
    """-> packed (N/4, C) uint8 [bits 2h..2h+1 of byte [k][c] = row 4k+h], scale (1,C), min (1,C).  The native INT2_MINMAX wire codec
    at residual 0; a channel whose values are all equal gets scale 0 and codes 0 (sim_int2_minmax returns NaN there)."""
    x = _nc(input_tensor)
    N, C = x.shape
    assert N % 4 == 0, f"Dimension N (0) size must be a multiple of 4 for INT2_MINMAX packing, got {N}"
    pkt, _ = codecs.compress(K.INT2_MINMAX, x, None, N, C, update_cache=False)
    qh = N * C // 8
    return pkt[:qh].view(torch.uint8).view(N // 4, C), pkt[qh:qh + C].view(1, C), pkt[qh + C:].view(1, C)


def dequantize_int2_minmax(packed_tensor: torch.Tensor, scale: torch.Tensor, min_val: torch.Tensor):
    assert packed_tensor.dtype == torch.uint8 and scale.dtype == torch.half and min_val.dtype == torch.half
    N4, C = packed_tensor.shape
    return codecs.decompress(K.INT2_MINMAX, _cat_packet(packed_tensor, scale, min_val), None, N4 * 4, C)


# ---- MXFP4 (extension: not in the reference; include/cfx.h "MXFP4") -----------------------------------------------
def quantize_mxfp4(input_tensor: torch.Tensor):
    """-> codes (N, C/2) uint8 [byte [n][j] = code[n][2j] | code[n][2j+1] << 4, code = sign << 3 | E2M1 index], scales (N, C/32) uint8
    [one E8M0 byte per block of 32 consecutive elements of a row; 0xFF: a block with a NaN or an inf].  The native MXFP4 wire codec at
    residual 0."""
    x = _nc(input_tensor)
    N, C = x.shape
    assert C % 64 == 0, f"Dimension C (1) size must be a multiple of 64 for MXFP4 blocks, got {C}"
    pkt, _ = codecs.compress(K.MXFP4, x, None, N, C, update_cache=False)
    by = pkt.view(torch.uint8)
    return by[:N * C // 2].view(N, C // 2), by[N * C // 2:].view(N, C // 32)


def dequantize_mxfp4(codes: torch.Tensor, scales: torch.Tensor):
    assert codes.dtype == torch.uint8 and scales.dtype == torch.uint8
    N, C2 = codes.shape
    assert scales.shape == (N, C2 // 16)
    return codecs.decompress(K.MXFP4, _cat_packet(codes, scales), None, N, C2 * 2)


def sim_mxfp4(input_tensor: torch.Tensor):
    return dequantize_mxfp4(*quantize_mxfp4(input_tensor))


# ---- BINARY_BLOCK (extension: not in the reference; include/cfx.h "BINARY_BLOCK") -----------------------------------
def quantize_binary_block(input_tensor: torch.Tensor, block: int = 64):
    """-> bits (N, C/8) uint8 [bit i of byte [n][j] = x[n][8j+i] >= 0], scales (N, C/block) fp16 [the abs-mean of each block of `block`
    consecutive elements of a row].  The native BINARY_BLOCK wire codec at residual 0."""
    x = _nc(input_tensor)
    N, C = x.shape
    assert block in (32, 64, 128), f"block size must be 32, 64 or 128, got {block}"
    assert C % max(block, 64) == 0, f"Dimension C (1) size must be a multiple of {max(block, 64)} for blocks of {block}, got {C}"
    pkt, _ = codecs.compress(K.BINARY_BLOCK, x, None, N, C, block, update_cache=False)
    return pkt[:N * C // 16].view(torch.uint8).view(N, C // 8), pkt[N * C // 16:].view(N, C // block)


def dequantize_binary_block(bits: torch.Tensor, scales: torch.Tensor):
    assert bits.dtype == torch.uint8 and scales.dtype == torch.half
    N, C8 = bits.shape
    C = C8 * 8
    block = C // scales.shape[1]
    assert scales.shape[0] == N and block in (32, 64, 128) and scales.shape[1] * block == C
    return codecs.decompress(K.BINARY_BLOCK, _cat_packet(bits, scales), None, N, C, block)


def sim_binary_block(input_tensor: torch.Tensor, block: int = 64):
    return dequantize_binary_block(*quantize_binary_block(input_tensor, block))


# ---- INT2_BLOCK (extension: not in the reference; include/cfx.h "INT2_BLOCK") ---------------------------------------
def quantize_int2_block(input_tensor: torch.Tensor, block: int = 64):
    """-> codes (N, C/4) uint8 [INT2's layout: bits 2i, 2i+1 of byte [n][j] = (x[n][4j+i] >= 0) << 1 | (|x[n][4j+i]| > scale)], scales
    (N, C/block) fp16 [the abs-mean of each block of `block` consecutive elements of a row].  The native INT2_BLOCK wire codec at residual 0."""
    x = _nc(input_tensor)
    N, C = x.shape
    assert block in (32, 64, 128), f"block size must be 32, 64 or 128, got {block}"
    assert C % max(block, 64) == 0, f"Dimension C (1) size must be a multiple of {max(block, 64)} for blocks of {block}, got {C}"
    pkt, _ = codecs.compress(K.INT2_BLOCK, x, None, N, C, block, update_cache=False)
    return pkt[:N * C // 8].view(torch.uint8).view(N, C // 4), pkt[N * C // 8:].view(N, C // block)


def dequantize_int2_block(codes: torch.Tensor, scales: torch.Tensor):
    assert codes.dtype == torch.uint8 and scales.dtype == torch.half
    N, C4 = codes.shape
    C = C4 * 4
    block = C // scales.shape[1]
    assert scales.shape[0] == N and block in (32, 64, 128) and scales.shape[1] * block == C
    return codecs.decompress(K.INT2_BLOCK, _cat_packet(codes, scales), None, N, C, block)


def sim_int2_block(input_tensor: torch.Tensor, block: int = 64):
    return dequantize_int2_block(*quantize_int2_block(input_tensor, block))


# ---- INT3_BLOCK (extension: not in the reference; include/cfx.h "INT3_BLOCK") ---------------------------------------
def quantize_int3_block(input_tensor: torch.Tensor, block: int = 64):
    """-> hi (N, C/4) uint8 [INT2's layout: bits 2i, 2i+1 of byte [n][j] = (x[n][4j+i] >= 0) << 1 | mag >> 1], lo (N, C/8) uint8 [BINARY's
    layout: bit i of byte [n][j] = mag & 1 of x[n][8j+i]], scales (N, C/block) fp16 [the abs-mean of each block of `block` consecutive
    elements of a row]; mag = 0..3 counts the thresholds 0.75 / 1.5 / 2.625 x scale that |x| exceeds.  The native INT3_BLOCK wire codec
    at residual 0."""
    x = _nc(input_tensor)
    N, C = x.shape
    assert block in (32, 64, 128), f"block size must be 32, 64 or 128, got {block}"
    assert C % max(block, 64) == 0, f"Dimension C (1) size must be a multiple of {max(block, 64)} for blocks of {block}, got {C}"
    pkt, _ = codecs.compress(K.INT3_BLOCK, x, None, N, C, block, update_cache=False)
    raw = pkt.view(torch.uint8)
    return raw[:N * C // 4].view(N, C // 4), raw[N * C // 4:3 * N * C // 8].view(N, C // 8), pkt[3 * N * C // 16:].view(N, C // block)


def dequantize_int3_block(hi: torch.Tensor, lo: torch.Tensor, scales: torch.Tensor):
    assert hi.dtype == torch.uint8 and lo.dtype == torch.uint8 and scales.dtype == torch.half
    N, C4 = hi.shape
    C = C4 * 4
    block = C // scales.shape[1]
    assert lo.shape == (N, C // 8) and scales.shape[0] == N and block in (32, 64, 128) and scales.shape[1] * block == C
    return codecs.decompress(K.INT3_BLOCK, _cat_packet(hi, lo, scales), None, N, C, block)


def sim_int3_block(input_tensor: torch.Tensor, block: int = 64):
    return dequantize_int3_block(*quantize_int3_block(input_tensor, block))


# ---- MXINT8 (extension: not in the reference; include/cfx.h "MXINT8") -----------------------------------------------
def quantize_mxint8(input_tensor: torch.Tensor):
    """-> codes (N, C) int8 [q = clamp(rne(x * 2^(6-X)), -127, 127)], scales (N, C/32) uint8 [one E8M0 byte X + 127 per block of 32
    consecutive elements of a row; 0xFF: a block with a NaN or an inf].  The native MXINT8 wire codec at residual 0."""
    x = _nc(input_tensor)
    N, C = x.shape
    assert C % 64 == 0, f"Dimension C (1) size must be a multiple of 64 for MXINT8 blocks, got {C}"
    pkt, _ = codecs.compress(K.MXINT8, x, None, N, C, update_cache=False)
    by = pkt.view(torch.uint8)
    return by[:N * C].view(torch.int8).view(N, C), by[N * C:].view(N, C // 32)


def dequantize_mxint8(codes: torch.Tensor, scales: torch.Tensor):
    assert codes.dtype == torch.int8 and scales.dtype == torch.uint8
    N, C = codes.shape
    assert scales.shape == (N, C // 32)
    return codecs.decompress(K.MXINT8, _cat_packet(codes, scales), None, N, C)


def sim_mxint8(input_tensor: torch.Tensor):
    return dequantize_mxint8(*quantize_mxint8(input_tensor))


def sim_int4(input_tensor: torch.Tensor, dim):
    x = _nc(input_tensor)
    if dim == 1:
        return sim_int4(x.t().contiguous(), 0).t().contiguous()
    return dequantize_int4(*quantize_int4(x))
