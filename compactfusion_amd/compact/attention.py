"""Block attention + running log-sum-exp merge used by the ring / gather consumers.

The reference takes these from un-vendored third-party packages (`yunchang.ring.utils.update_out_and_lse`,
`yunchang.kernels.attention.pytorch_attn_forward`, `flash_attn._flash_attn_forward`; call sites ring.py:225-263).
They are restated here from the published ring-attention algorithm:
    out <- out - sigmoid(lse_b - lse) * (out - out_b) ;  lse <- lse - logsigmoid(lse - lse_b)
The attention math itself is not part of the compressed-exchange hot path; on the GPU it is PyTorch-ROCm's fused
SDPA kernel, elsewhere an explicit fp32 softmax.  Opt-in (configure(attention="native")): `attention_blocks`, ONE native launch
over all of a layer's K,V blocks where they lie (cfx_attn_fwd_blocks; head dims 72 .. 120: cfx_attn_fwd_blocks_hd) in place of W SDPA
calls and their merge."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn.functional as F


def block_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, dropout_p: float = 0.0,
                    softmax_scale: Optional[float] = None, causal: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """q (B, Sq, H, D), k/v (B, Sk, H, D) -> out (B, Sq, H, D) in q.dtype, lse (B, H, Sq) fp32."""
    if softmax_scale is None:
        softmax_scale = q.shape[-1] ** (-0.5)
    qt, kt, vt = (t.transpose(1, 2) for t in (q, k, v))
    if q.is_cuda and dropout_p == 0.0:
        try:
            res = torch.ops.aten._scaled_dot_product_flash_attention(qt, kt, vt, 0.0, causal, False, scale=softmax_scale)
            return res[0].transpose(1, 2), res[1].float()
        except (RuntimeError, NotImplementedError):
            pass
    s = torch.matmul(qt.float(), kt.float().transpose(-1, -2)) * softmax_scale
    if causal:
        Sq, Sk = s.shape[-2], s.shape[-1]
        mask = torch.ones(Sq, Sk, dtype=torch.bool, device=s.device).tril(diagonal=Sk - Sq)
        s = s.masked_fill(~mask, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.unsqueeze(-1))
    if dropout_p > 0.0:
        p = F.dropout(p, dropout_p)
    out = torch.matmul(p, vt.float()).to(q.dtype)
    return out.transpose(1, 2), lse


def update_out_and_lse(out: Optional[torch.Tensor], lse: Optional[torch.Tensor], block_out: torch.Tensor,
                       block_lse: torch.Tensor, wait=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Merge one attention block into the running (out fp32 (B,S,H,D), lse fp32 (B,S,H,1)).  On the GPU this is ONE native
    launch (`cfx_attn_merge_ex`; fp16 or bf16 blocks) that reads the SDPA kernel's own (B,H,S,D) / (B,H,S) outputs and updates
    out / lse in place; elsewhere (CPU tests of the host logic) the same formula in eager torch.
    `wait` = (flag device address, epoch): the exchange lane's "next peer reconstructed" flag - the merge launch also waits for
    it, so the attention block that follows finds the peer's K,V complete without a stream event."""
    if block_out.is_cuda and block_out.dtype in (torch.float16, torch.bfloat16) and block_lse.dtype == torch.float32 and block_out.shape[-1] % 8 == 0 \
            and block_out.shape[-1] <= 512 and (out is None or (out.is_contiguous() and lse.is_contiguous() and out.dtype == torch.float32)):
        if block_lse.is_contiguous() and block_out.data_ptr() % 16 == 0:
            if block_out.is_contiguous():                  # the fused SDPA output, (B,S,H,D) contiguous underneath
                return _merge_native(out, lse, block_out, block_lse, 1, wait)
            if block_out.transpose(1, 2).is_contiguous():  # ... or (B,H,S,D)
                return _merge_native(out, lse, block_out, block_lse, 0, wait)
    block_out = block_out.to(torch.float32)
    block_lse = block_lse.transpose(-2, -1).unsqueeze(-1)
    if out is not None:
        out = out - torch.sigmoid(block_lse - lse) * (out - block_out)
        lse = lse - F.logsigmoid(lse - block_lse)
    else:
        out, lse = block_out, block_lse
    if wait is not None:
        flag_wait(wait, block_out.device)
    return out, lse


def merge_blocks(block_outs, block_lses, out_dtype=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """ALL of a layer's attention blocks merged at once: block_outs[i] (B, S, H, D), block_lses[i] fp32 (B, H, S) - what
    `block_attention` returns - -> out (B, S, H, D) in `out_dtype` (fp32 when None), lse fp32 (B, S, H, 1).  The softmax-weighted
    combination is formed directly, not as the chain `update_out_and_lse` runs (include/cfx.h, cfx_attn_merge_many, states it rounding
    by rounding):
        m = max_i lse_i ;  e_i = exp(lse_i - m) ;  Z = sum_i e_i ;  out = (sum_i e_i out_i) / Z ;  lse = m + log Z
    On the GPU - fp16 or bf16 blocks, D % 8 == 0, D <= 512, every block in the same one of the two layouts the fused SDPA op returns,
    out_dtype fp32 or the blocks' type - this is ONE native launch.  The launch takes at most 16 blocks: more on the native path are
    REFUSED (ValueError) - they are neither folded through a second launch, whose intermediate would round where the formula above does
    not, nor handed to eager torch behind the caller's back.  Anything else (CPU tensors: the host-logic tests; other layouts or
    types) runs the same direct formula in eager fp32 torch - never the chain."""
    n = len(block_outs)
    if n == 0 or n != len(block_lses):
        raise ValueError(f"merge_blocks: {n} block outputs, {len(block_lses)} block lse tensors")
    bo0 = block_outs[0]
    if out_dtype is None:
        out_dtype = torch.float32
    if bo0.is_cuda and bo0.dim() == 4 and bo0.dtype in (torch.float16, torch.bfloat16) and out_dtype in (torch.float32, bo0.dtype) \
            and bo0.shape[-1] % 8 == 0 and bo0.shape[-1] <= 512:
        bshd = 1 if bo0.is_contiguous() else (0 if bo0.transpose(1, 2).is_contiguous() else None)
        if bshd is not None and all(
                bo.shape == bo0.shape and bo.dtype == bo0.dtype and bo.device == bo0.device and bo.data_ptr() % 16 == 0
                and (bo.is_contiguous() if bshd else bo.transpose(1, 2).is_contiguous())
                and bl.dtype == torch.float32 and bl.is_contiguous() and bl.device == bo0.device
                and bl.shape == (bo0.shape[0], bo0.shape[2], bo0.shape[1]) for bo, bl in zip(block_outs, block_lses)):
            from .. import _lib
            if n > _lib.MERGE_MAX_BLOCKS:
                raise ValueError(f"merge_blocks: {n} blocks - the one-launch merge takes at most {_lib.MERGE_MAX_BLOCKS} "
                                 "(configure(attn_merge='chain') merges any number)")
            return _merge_many_native(block_outs, block_lses, bshd, out_dtype)
    return _merge_direct([bo.to(torch.float32) for bo in block_outs],
                         [bl.to(torch.float32).transpose(-2, -1).unsqueeze(-1) for bl in block_lses], out_dtype)


def _merge_direct(outs, lses, out_dtype):
    """the direct formula in eager fp32 torch: outs[i] fp32 (B, S, H, D), lses[i] fp32 (B, S, H, 1); sums in index order"""
    m = lses[0]
    for l in lses[1:]:
        m = torch.maximum(m, l)
    acc = z = None
    for o, l in zip(outs, lses):
        e = torch.exp(l - m)
        acc, z = (e * o, e) if acc is None else (acc + e * o, z + e)
    return (acc / z).to(out_dtype), m + torch.log(z)


_merge_many_fn = None


def _merge_many_native(block_outs, block_lses, bshd, out_dtype):
    global _merge_many_fn
    import ctypes
    from .. import _lib, codecs
    bo0 = block_outs[0]
    n = len(block_outs)
    B, S, H, D = bo0.shape
    dev = bo0.device.index if bo0.device.index is not None else torch.cuda.current_device()
    if _merge_many_fn is None:
        _merge_many_fn = _lib.load().cfx_attn_merge_many
    out = torch.empty((B, S, H, D), dtype=out_dtype, device=bo0.device)
    lse = torch.empty((B, S, H, 1), dtype=torch.float32, device=bo0.device)
    ctx = codecs.context(dev)
    flags = (_lib.MERGE_BSHD if bshd else 0) | (_lib.ELEM_BF16 if bo0.dtype == torch.bfloat16 else 0) \
        | (_lib.MERGE_OUT_F32 if out_dtype == torch.float32 else 0)
    P = ctypes.c_void_p * n
    rc = _merge_many_fn(ctx, n, P(*[t.data_ptr() for t in block_outs]), P(*[t.data_ptr() for t in block_lses]), B, S, H, D, flags,
                        out.data_ptr(), lse.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        codecs._check(ctx, rc, "cfx_attn_merge_many")
    return out, lse


def attention_blocks(q, ks, vs, softmax_scale: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The attention of q (B, Sq, H, D) over ALL the K,V blocks ks[i], vs[i] (B, Sk, H, D) - non-causal, no dropout - as if they were
    one sequence: out (B, Sq, H, D) in q.dtype, lse fp32 as the (B, H, Sq) view of a (B, Sq, H) tensor.  Nothing is concatenated and no
    per-block out / lse exists (include/cfx.h, cfx_attn_fwd_blocks, states the arithmetic rounding by rounding).
    On the GPU - q and every block fp16 or bf16 alike, contiguous, 16-byte aligned, on one device, D one of ATTN_HEAD_DIMS (64, 128 and
    the multiples of 8 between them), the blocks agreeing with q in B, H and D - this is ONE native launch: at D 64 or 128
    cfx_attn_fwd_blocks for blocks of one shape and cfx_attn_fwd_blocks_var for blocks that differ in their key count (ks[i]
    (B, Sk_i, H, D)); at D 72 .. 120 cfx_attn_fwd_blocks_hd for both.  The launch takes at most 16 blocks: more on the native path are
    REFUSED (ValueError), as `merge_blocks` refuses them.  Anything else (CPU tensors: the host-logic tests; other types, head dims or
    layouts) runs the direct definition in eager fp32 torch."""
    n = len(ks)
    if n == 0 or n != len(vs):
        raise ValueError(f"attention_blocks: {n} K blocks, {len(vs)} V blocks")
    if softmax_scale is None:
        softmax_scale = q.shape[-1] ** (-0.5)
    if attn_native_ok(q, ks, vs):
        from .. import _lib
        if n > _lib.ATTN_MAX_BLOCKS:
            raise ValueError(f"attention_blocks: {n} blocks - the one-launch attention takes at most {_lib.ATTN_MAX_BLOCKS} "
                             "(configure(attention='sdpa') attends to any number)")
        return _attn_fwd_native(q, ks, vs, softmax_scale)
    if attn_native_var_ok(q, ks, vs):                                                         # blocks that differ in their key count only
        from .. import _lib
        if n > _lib.ATTN_MAX_BLOCKS:
            raise ValueError(f"attention_blocks: {n} blocks - the one-launch attention takes at most {_lib.ATTN_MAX_BLOCKS} "
                             "(configure(attention='sdpa') attends to any number)")
        return _attn_fwd_native_var(q, ks, vs, softmax_scale)
    qt = q.float().transpose(1, 2)                                                            # (B, H, Sq, D)
    s = torch.cat([torch.matmul(qt, k.float().permute(0, 2, 3, 1)) for k in ks], dim=-1) * softmax_scale
    m = s.max(dim=-1, keepdim=True).values
    p = torch.exp(s - m)
    l = p.sum(dim=-1, keepdim=True)
    out = torch.matmul(p, torch.cat([v.float().transpose(1, 2) for v in vs], dim=-2)) / l
    lse = torch.empty((q.shape[0], q.shape[1], q.shape[2]), dtype=torch.float32, device=q.device)   # (B, Sq, H), as the launch stores it
    lse.copy_((m + torch.log(l)).squeeze(-1).transpose(1, 2))
    return out.transpose(1, 2).contiguous().to(q.dtype), lse.transpose(1, 2)


ATTN_HEAD_DIMS = (64, 72, 80, 88, 96, 104, 112, 120, 128)      # 64, 128: cfx_attn_fwd_blocks / _var; between them: cfx_attn_fwd_blocks_hd


def attn_native_ok(q, ks, vs) -> bool:
    """whether `attention_blocks` takes (q, ks, vs) to the native launch (the number of blocks aside)"""
    if not (q.is_cuda and q.dim() == 4 and q.dtype in (torch.float16, torch.bfloat16) and q.shape[-1] in ATTN_HEAD_DIMS
            and q.is_contiguous() and q.data_ptr() % 16 == 0 and q.shape[1] > 0):
        return False
    k0 = ks[0]
    if k0.dim() != 4 or k0.shape[1] <= 0 or (k0.shape[0], k0.shape[2], k0.shape[3]) != (q.shape[0], q.shape[2], q.shape[3]):
        return False
    return all(t.shape == k0.shape and t.dtype == q.dtype and t.device == q.device and t.is_contiguous() and t.data_ptr() % 16 == 0
               for t in list(ks) + list(vs))


def attn_native_var_ok(q, ks, vs) -> bool:
    """whether `attention_blocks` takes (q, ks, vs) to the native launch for blocks of unequal length (cfx_attn_fwd_blocks_var, at head
    dims 72 .. 120 cfx_attn_fwd_blocks_hd; the number of blocks aside): `attn_native_ok`'s conditions block by block - K and V of a block of one shape - with the key count free"""
    return len(ks) == len(vs) and all(k.dim() == 4 and k.shape == v.shape and attn_native_ok(q, (k,), (v,)) for k, v in zip(ks, vs))


_attn_fwd_fn = None
_attn_var_fn = None
_attn_hd_fn = None


def _attn_fwd_native(q, ks, vs, softmax_scale, tabs=None):
    """the launch itself, on arguments `attn_native_ok` passed; `tabs`: the caller's two ctypes pointer tables (compact/ring.py keeps
    a layer's), built here otherwise.  A head dim between 64 and 128 goes to cfx_attn_fwd_blocks_hd, which has the unequal-length form
    only: its key-count table is Sk n times."""
    global _attn_fwd_fn
    import ctypes
    from .. import _lib, codecs
    n = len(ks)
    B, Sq, H, D = q.shape
    if D not in (64, 128):
        if tabs is None:
            P = ctypes.c_void_p * n
            tabs = P(*[t.data_ptr() for t in ks]), P(*[t.data_ptr() for t in vs])
        return _attn_fwd_native_var(q, ks, vs, softmax_scale, (tabs[0], tabs[1], (ctypes.c_int * n)(*([ks[0].shape[1]] * n))))
    dev = q.device.index if q.device.index is not None else torch.cuda.current_device()
    if _attn_fwd_fn is None:
        _attn_fwd_fn = _lib.load().cfx_attn_fwd_blocks
    if tabs is None:
        P = ctypes.c_void_p * n
        tabs = P(*[t.data_ptr() for t in ks]), P(*[t.data_ptr() for t in vs])
    out = torch.empty((B, Sq, H, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, Sq, H), dtype=torch.float32, device=q.device)
    ctx = codecs.context(dev)
    rc = _attn_fwd_fn(ctx, n, q.data_ptr(), tabs[0], tabs[1], B, Sq, ks[0].shape[1], H, D, softmax_scale,
                      _lib.ELEM_BF16 if q.dtype == torch.bfloat16 else 0, out.data_ptr(), lse.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        codecs._check(ctx, rc, "cfx_attn_fwd_blocks")
    return out, lse.transpose(1, 2)


def _attn_fwd_native_var(q, ks, vs, softmax_scale, tabs=None):
    """the launch for blocks of unequal length, on arguments `attn_native_var_ok` passed; `tabs`: the caller's three ctypes tables - K
    pointers, V pointers, key counts (compact/ring.py keeps a layer's) -, built here otherwise.  D 64 or 128: cfx_attn_fwd_blocks_var;
    a head dim between them: cfx_attn_fwd_blocks_hd, the same arguments"""
    global _attn_var_fn, _attn_hd_fn
    import ctypes
    from .. import _lib, codecs
    n = len(ks)
    B, Sq, H, D = q.shape
    dev = q.device.index if q.device.index is not None else torch.cuda.current_device()
    if _attn_var_fn is None:
        _attn_var_fn, _attn_hd_fn = _lib.load().cfx_attn_fwd_blocks_var, _lib.load().cfx_attn_fwd_blocks_hd
    fn, name = (_attn_var_fn, "cfx_attn_fwd_blocks_var") if D in (64, 128) else (_attn_hd_fn, "cfx_attn_fwd_blocks_hd")
    if tabs is None:
        P = ctypes.c_void_p * n
        tabs = P(*[t.data_ptr() for t in ks]), P(*[t.data_ptr() for t in vs]), (ctypes.c_int * n)(*[t.shape[1] for t in ks])
    out = torch.empty((B, Sq, H, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, Sq, H), dtype=torch.float32, device=q.device)
    ctx = codecs.context(dev)
    rc = fn(ctx, n, q.data_ptr(), tabs[0], tabs[1], tabs[2], B, Sq, H, D, softmax_scale,
                      _lib.ELEM_BF16 if q.dtype == torch.bfloat16 else 0, out.data_ptr(), lse.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        codecs._check(ctx, rc, name)
    return out, lse.transpose(1, 2)


def attn_fwd_launches(device=None) -> int:
    """cfx_attn_fwd_blocks / cfx_attn_fwd_blocks_var / cfx_attn_fwd_blocks_hd launches enqueued so far on the device's context (the launch carries no kernel id: the context counts)"""
    import ctypes
    from .. import _lib, codecs
    dev = torch.cuda.current_device() if device is None else (device.index if isinstance(device, torch.device) else device)
    n = ctypes.c_ulonglong(0)
    ctx = codecs.context(dev)
    rc = _lib.load().cfx_attn_fwd_launches(ctx, ctypes.byref(n))
    if rc != 0:
        codecs._check(ctx, rc, "cfx_attn_fwd_launches")
    return int(n.value)


def flag_wait(wait, device) -> None:
    """A stand-alone wait launch on the current stream for (flag address, epoch) - what `update_out_and_lse(wait=...)` folds into
    its merge launch when it can."""
    from .. import _lib, codecs
    dev = device.index if device.index is not None else torch.cuda.current_device()
    ctx = codecs.context(dev)
    rc = _lib.load().cfx_flag_wait(ctx, wait[0], wait[1], torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        codecs._check(ctx, rc, "cfx_flag_wait")


_merge_fn = None


def _merge_native(out, lse, bo, bl, bshd, wait=None):
    global _merge_fn
    from .. import _lib, codecs
    B, S, H, D = bo.shape
    dev = bo.device.index if bo.device.index is not None else torch.cuda.current_device()
    first = out is None
    if first:
        out = torch.empty((B, S, H, D), dtype=torch.float32, device=bo.device)
        lse = torch.empty((B, S, H, 1), dtype=torch.float32, device=bo.device)
    if _merge_fn is None:
        _merge_fn = _lib.load().cfx_attn_merge_ex
    ctx = codecs.context(dev)
    flags = (_lib.MERGE_BSHD if bshd else 0) | (_lib.MERGE_FIRST if first else 0) | (_lib.ELEM_BF16 if bo.dtype == torch.bfloat16 else 0)
    rc = _merge_fn(ctx, out.data_ptr(), lse.data_ptr(), bo.data_ptr(), bl.data_ptr(), B, S, H, D, flags,
                   wait[0] if wait is not None else None, wait[1] if wait is not None else 0, None,
                   torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        codecs._check(ctx, rc, "cfx_attn_merge_ex")
    return out, lse
