"""The bf16 numerics contract of the 1-bit and 2-bit exchange (include/cfx.h, "bf16 activations"), stated on top of the pinned oracle
(oracle/ref_np.py) - a helper, not a test.  Activations and states are bf16; the residual domain and the wire stay fp16:

    d        = fp16_rne( fp32(x) - fp32(base) )                  base None: fp16_rne(fp32(x))
    pkt, recv = oracle.compress(codec, d, None, param)           everything between d and recv is the fp16 path
    new_base = recon = bf16_rne( fp32(base) + fp32(recv) )       base None: bf16_rne(fp32(recv));  error feedback off: new_base = x

bf16 tensors are uint16 bit patterns here (numpy has no bf16): bf16 -> fp32 is a shift, fp32 -> bf16 rounds to nearest even exactly
like `tensor.to(torch.bfloat16)` does for finite values."""
import numpy as np

from oracle import ref_np as R

NAMES = {1: "binary", 2: "int2"}
ELEM_BF16 = 0x100


def bf16_to_f32(u16):
    return (np.ascontiguousarray(u16).astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16(f32):
    """Round to nearest even (finite values)."""
    u = np.ascontiguousarray(f32, dtype=np.float32).view(np.uint32)
    return ((u + (0x7FFF + ((u >> 16) & 1))) >> 16).astype(np.uint16)


def delta(x_u16, base_u16):
    with np.errstate(over="ignore"):
        d = bf16_to_f32(x_u16) if base_u16 is None else bf16_to_f32(x_u16) - bf16_to_f32(base_u16)
        return d.astype(np.float16)


def add_base(base_u16, recv16):
    r = R.as_f16(recv16).astype(np.float32)
    return f32_to_bf16(r if base_u16 is None else bf16_to_f32(base_u16) + r)


def compress(name, x_u16, base_u16, param=0, ef=True):
    """(packet words uint16, new_base bf16 bits)"""
    pkt, recv = R.compress(name, delta(x_u16, base_u16), None, param)
    nb = add_base(base_u16, recv) if ef else np.array(x_u16, dtype=np.uint16, copy=True)
    return pkt, nb


def decompress(name, pkt, base_u16, N, C, param=0):
    """recon bf16 bits"""
    return add_base(base_u16, R.decompress(name, pkt, N, C, param))


def int2_quantize(x_u16, base_u16, tok16, chan16):
    """cfx_int2_quantize with CFX_FLAG_ELEM_BF16: the scales are GIVEN (the packet tail); (packet words, new_base bf16 bits)"""
    d = delta(x_u16, base_u16)
    idx, thr = R.int2_codes(d, R.as_f16(tok16), R.as_f16(chan16))
    pkt = R.fastpath_packet(R.pack_int2(idx), R.as_f16(tok16), R.as_f16(chan16))
    return pkt, add_base(base_u16, R.int2_levels(idx, thr))


def torch_bits(t):
    """uint16 bit patterns of a 16-bit torch tensor (fp16 or bf16), on the host."""
    import torch
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)
