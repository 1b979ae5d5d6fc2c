"""The block-merge kernels against the float64 formula within the derived bound of tests/_merge_f64.py, over the head dims, row counts,
chain lengths, lse gaps and value ranges the C-ABI accepts (GPU box only, -m gpu): cfx_attn_merge, cfx_attn_merge_wait and
cfx_attn_merge_ex (non-final) - for fp16 blocks the three equal bit for bit -, the final cast in the launch against torch's cast of the
stored fp32 value, and FIRST | final_out.  Both block layouts inside every chain.  Every case prints the worst error of the kernel and
of the eager fp32 formula as a fraction of the bound (docs/DESIGN_DETAIL.md keeps the figures per gap class)."""
import numpy as np
import pytest
import torch

import _merge_f64 as M

pytestmark = pytest.mark.gpu
BSHD, FIRST, BF = 1, 2, 0x100


def _lib_ctx():
    from compactfusion_amd import _lib, codecs as K
    return _lib.load(), K.context(0)


def _same_bits(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    v = torch.int16 if a.element_size() == 2 else torch.int32
    return torch.equal(a.contiguous().view(v), b.contiguous().view(v))


def to_device(case, blocks):
    """[(block_out, block_lse (B,H,S), bshd)]: even blocks [B][S][H][D], odd blocks [B][H][S][D] underneath"""
    dt = torch.float16 if case["dtype"] == "fp16" else torch.bfloat16
    out = []
    for k, (ob, lb) in enumerate(blocks):
        t = torch.from_numpy(ob).to(dt)
        assert torch.equal(t.float(), torch.from_numpy(ob))
        bshd = k % 2 == 0
        t = t.cuda() if bshd else t.permute(0, 2, 1, 3).contiguous().cuda()
        out.append((t, torch.from_numpy(lb).transpose(1, 2).contiguous().cuda(), int(bshd)))
    return out


def chain(case, dblocks, entry, final=False):
    """merge dblocks in order through one entry point; final: the last launch writes the 16-bit result.  (out32, lse, final_out | None)"""
    lib, ctx = _lib_ctx()
    B, S, H, D = case["shape"]
    dt = dblocks[0][0].dtype
    elem = BF if dt == torch.bfloat16 else 0
    out = torch.full((B, S, H, D), float("nan"), dtype=torch.float32, device="cuda")
    lse = torch.full((B, S, H), float("nan"), dtype=torch.float32, device="cuda")
    fin = torch.full((B, S, H, D), float("nan"), dtype=dt, device="cuda") if final else None
    flag = torch.full((16,), 7, dtype=torch.int32, device="cuda")
    sh = torch.cuda.current_stream().cuda_stream
    for i, (bo, bl, bshd) in enumerate(dblocks):
        first = int(i == 0)
        if entry == "merge":
            rc = lib.cfx_attn_merge(ctx, out.data_ptr(), lse.data_ptr(), bo.data_ptr(), bl.data_ptr(), B, S, H, D, bshd, first, sh)
        elif entry == "wait":           # (the flag has arrived: the launch's one polling lane returns at once)
            rc = lib.cfx_attn_merge_wait(ctx, out.data_ptr(), lse.data_ptr(), bo.data_ptr(), bl.data_ptr(), B, S, H, D, bshd, first, flag.data_ptr(), 7, sh)
        else:
            last = final and i == len(dblocks) - 1
            rc = lib.cfx_attn_merge_ex(ctx, out.data_ptr(), lse.data_ptr(), bo.data_ptr(), bl.data_ptr(), B, S, H, D,
                                       elem | (BSHD if bshd else 0) | (FIRST if first else 0), None, 0, fin.data_ptr() if last else None, sh)
        assert rc == 0, lib.cfx_last_error_string(ctx)
    torch.cuda.synchronize()
    return out, lse, fin


@pytest.mark.parametrize("case", M.CASES, ids=[c["id"] for c in M.CASES])
def test_merge_kernels_meet_the_float64_bound(case):
    lib, ctx = _lib_ctx()
    blocks = M.build(case)
    db = to_device(case, blocks)
    B, S, H, D = case["shape"]
    out, lse, _ = chain(case, db, "ex")
    ko, kl = M.check(out.cpu().numpy(), lse.cpu().numpy(), blocks, "cfx_attn_merge_ex")
    eo, el = M.check(*M.eager_fp32(blocks), blocks, "eager fp32 formula")
    print(f"MERGE-ERR {case['gap']} {case['id']} kernel {ko:.4f} {kl:.4f} eager {eo:.4f} {el:.4f}")
    if case["dtype"] == "fp16":
        for entry in ("merge", "wait"):
            o2, l2, _ = chain(case, db, entry)
            assert _same_bits(o2, out) and _same_bits(l2, lse), f"cfx_attn_merge{'_wait' if entry == 'wait' else ''} differs from cfx_attn_merge_ex"
    # the final cast in the launch
    want = out.to(db[0][0].dtype)
    o_f, l_f, fin = chain(case, db, "ex", final=True)
    before, _, _ = chain(case, db[:-1], "ex")
    assert _same_bits(fin, want), f"final_out: {int((fin.view(torch.int16) != want.view(torch.int16)).sum())} elements differ from the cast of the stored fp32 value"
    assert _same_bits(l_f, lse), "lse of the final launch"
    assert _same_bits(o_f, before), "the final launch wrote the fp32 out"
    # FIRST | final_out, out NULL: the block's own bits (both layouts)
    for bo, bl, bshd in db[:2]:
        fin1 = torch.full((B, S, H, D), float("nan"), dtype=bo.dtype, device="cuda")
        lse1 = torch.full((B, S, H), float("nan"), dtype=torch.float32, device="cuda")
        elem = BF if bo.dtype == torch.bfloat16 else 0
        assert lib.cfx_attn_merge_ex(ctx, None, lse1.data_ptr(), bo.data_ptr(), bl.data_ptr(), B, S, H, D, elem | (BSHD if bshd else 0) | FIRST, None, 0,
                                     fin1.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0, lib.cfx_last_error_string(ctx)
        torch.cuda.synchronize()
        logical = bo if bshd else bo.permute(0, 2, 1, 3)
        assert _same_bits(fin1, logical.contiguous()) and _same_bits(lse1, bl.transpose(1, 2).contiguous())
    assert lib.cfx_gate_errors(ctx) == 0
