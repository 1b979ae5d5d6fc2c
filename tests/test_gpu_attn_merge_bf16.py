"""cfx_attn_merge_ex on the GPU (-m gpu): the ring-attention block merge for bf16 blocks, the layer's final cast inside the last merge
launch (fp16 and bf16), the lane's wait folded into such a launch, and compact_fwd's lean block loop for bf16 q, k, v.  Every case
fails on a library without the entry point."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bf16_contract as BC

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BSHD, FIRST, BF = 1, 2, 0x100
KID_ATTN_MERGE = 30
bits = BC.torch_bits


@pytest.fixture(autouse=True)
def _collector(tmp_path):
    from compactfusion_amd.collector import collector
    collector.init(collector.Collector(str(tmp_path), enabled=False))
    yield


def _lib_ctx():
    from compactfusion_amd import _lib, codecs as K
    return _lib.load(), K.context(0)


def _elem(dtype):
    return BF if dtype == torch.bfloat16 else 0


def _same_bits(a, b):
    """two tensors of one 16-bit or 32-bit type hold the same bits"""
    assert a.dtype == b.dtype and a.shape == b.shape
    v = torch.int16 if a.element_size() == 2 else torch.int32
    return torch.equal(a.contiguous().view(v), b.contiguous().view(v))


def _formula(ref_o, ref_l, bo, bl):
    """the published update_out_and_lse, written out in eager fp32"""
    bo32, bl4 = bo.to(torch.float32), bl.transpose(-2, -1).unsqueeze(-1)
    if ref_o is None:
        return bo32, bl4
    return ref_o - torch.sigmoid(bl4 - ref_l) * (ref_o - bo32), ref_l - F.logsigmoid(ref_l - bl4)


def _blocks(dtype, D, n=4, seed=3, B=2, S=77, H=5):
    """n attention blocks (out (B,S,H,D) in `dtype`, lse (B,H,S) fp32) from the fused SDPA kernel; block 2 in the other layout the merge reads"""
    from compactfusion_amd.compact import attention as A
    g = torch.Generator(device="cuda").manual_seed(seed)
    q = torch.randn(B, S, H, D, device="cuda", dtype=dtype, generator=g)
    out = []
    for blk in range(n):
        k = torch.randn(B, 40 + blk, H, D, device="cuda", dtype=dtype, generator=g) * (1 + blk)
        v = torch.randn(B, 40 + blk, H, D, device="cuda", dtype=dtype, generator=g)
        bo, bl = A.block_attention(q, k, v, 0.0, None, causal=False)
        assert bo.dtype == dtype and bl.dtype == torch.float32 and bl.is_contiguous()
        if blk == 2:
            bo = bo.transpose(1, 2).contiguous().transpose(1, 2)          # (B,H,S,D) underneath
        out.append((bo, bl))
    return out


def _bshd(bo):
    if bo.is_contiguous():
        return 1
    assert bo.transpose(1, 2).is_contiguous()
    return 0


# ---- 5: bf16 blocks against the published formula ------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 72, 96, 128, 160])
def test_native_merge_of_bf16_blocks_equals_the_eager_formula(D):
    """update_out_and_lse on bf16 blocks is ONE native launch per block (both block layouts), and equals the formula in eager fp32 torch
    to the tolerance the fp16 kernel is held to (test_gpu_api.py): the bf16 -> fp32 widening is exact, nothing else differs."""
    from compactfusion_amd.compact import attention as A
    out = lse = ref_o = ref_l = None
    layouts = set()
    for blk, (bo, bl) in enumerate(_blocks(torch.bfloat16, D)):
        calls = []
        orig = A._merge_native
        A._merge_native = lambda *a: (calls.append(a[4]), orig(*a))[1]
        try:
            out, lse = A.update_out_and_lse(out, lse, bo, bl)
        finally:
            A._merge_native = orig
        assert len(calls) == 1 and (blk != 2 or calls == [0]), "the native merge launch was not taken"
        layouts.add(calls[0])
        ref_o, ref_l = _formula(ref_o, ref_l, bo, bl)
    torch.cuda.synchronize()
    assert layouts == {0, 1}, "both block layouts"
    B, S, H = 2, 77, 5
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, S, H, D) and tuple(lse.shape) == (B, S, H, 1)
    print(f"D {D}: max |out - formula| {float((out - ref_o).abs().max()):.3e}, max |lse - formula| {float((lse - ref_l).abs().max()):.3e}")
    torch.testing.assert_close(out, ref_o, rtol=2e-6, atol=2e-6)
    torch.testing.assert_close(lse, ref_l, rtol=2e-6, atol=2e-6)
    lib, ctx = _lib_ctx()
    assert lib.cfx_gate_errors(ctx) == 0


# ---- 6: the final cast in the launch ---------------------------------------------------------------------------------------------------
def _chain(lib, ctx, blocks, dtype, final, old_call=False, stream=None):
    """Merge `blocks` in order.  final: the last block's launch writes the 16-bit result itself; otherwise all launches are the non-final
    form (old_call: cfx_attn_merge_wait, fp16 only).  Returns (out32, lse, final_out or None)."""
    B, S, H, D = blocks[0][0].shape
    out = torch.full((B, S, H, D), float("nan"), dtype=torch.float32, device="cuda")
    lse = torch.full((B, S, H, 1), float("nan"), dtype=torch.float32, device="cuda")
    fin = torch.full((B, S, H, D), float("nan"), dtype=dtype, device="cuda") if final else None
    sh = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    for i, (bo, bl) in enumerate(blocks):
        last = i == len(blocks) - 1
        if old_call:
            rc = lib.cfx_attn_merge_wait(ctx, out.data_ptr(), lse.data_ptr(), bo.data_ptr(), bl.data_ptr(), B, S, H, D, _bshd(bo), int(i == 0), None, 0, sh)
        else:
            flags = _elem(dtype) | (BSHD if _bshd(bo) else 0) | (FIRST if i == 0 else 0)
            rc = lib.cfx_attn_merge_ex(ctx, out.data_ptr(), lse.data_ptr(), bo.data_ptr(), bl.data_ptr(), B, S, H, D, flags, None, 0,
                                       fin.data_ptr() if final and last else None, sh)
        assert rc == 0, lib.cfx_last_error_string(ctx)
    return out, lse, fin


@pytest.mark.parametrize("D", [64, 72, 128, 160])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_final_cast_in_the_launch_is_the_cast_of_the_stored_value(dtype, D):
    """(a) every block merged by the non-final form - for fp16 by the EXISTING cfx_attn_merge_wait -, then out32.to(dtype) by torch;
    (b) the last block with final_out.  The 16-bit results and lse are equal bit for bit; (b)'s launch leaves the fp32 out as the block
    before left it.  A single block with FIRST | final_out (out NULL): final_out is the block's bits, lse the block's."""
    lib, ctx = _lib_ctx()
    blocks = _blocks(dtype, D)
    out_a, lse_a, _ = _chain(lib, ctx, blocks, dtype, final=False, old_call=dtype == torch.float16)
    want = out_a.to(dtype)
    out_b, lse_b, fin = _chain(lib, ctx, blocks, dtype, final=True)
    before, _, _ = _chain(lib, ctx, blocks[:-1], dtype, final=False)
    torch.cuda.synchronize()
    assert not torch.isnan(fin.float()).any() and not torch.isnan(lse_b).any()
    assert _same_bits(fin, want), f"{dtype} D {D}: {int((fin.view(torch.int16) != want.view(torch.int16)).sum())} elements differ"
    assert _same_bits(lse_b, lse_a)
    assert _same_bits(out_b, before), "the final launch wrote the fp32 out"
    if dtype == torch.float16:
        # the new entry point's non-final form against the existing call, too
        out_c, lse_c, _ = _chain(lib, ctx, blocks, dtype, final=False)
        torch.cuda.synchronize()
        assert _same_bits(out_c, out_a) and _same_bits(lse_c, lse_a)
    # one block
    for bo, bl in (blocks[0], blocks[2]):
        B, S, H, _ = bo.shape
        fin1 = torch.full((B, S, H, D), float("nan"), dtype=dtype, device="cuda")
        lse1 = torch.full((B, S, H, 1), float("nan"), dtype=torch.float32, device="cuda")
        flags = _elem(dtype) | (BSHD if _bshd(bo) else 0) | FIRST
        assert lib.cfx_attn_merge_ex(ctx, None, lse1.data_ptr(), bo.data_ptr(), bl.data_ptr(), B, S, H, D, flags, None, 0, fin1.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream) == 0, lib.cfx_last_error_string(ctx)
        torch.cuda.synchronize()
        assert _same_bits(fin1, bo.contiguous()) and _same_bits(lse1, bl.transpose(-2, -1).unsqueeze(-1).contiguous())
    assert lib.cfx_gate_errors(ctx) == 0


# ---- 7: the wait, folded into a bf16 / FINAL launch -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_merge_ex_wait_releases_when_the_flag_arrives(dtype):
    """Two launches on one stream: FIRST (non-final) waiting for epoch 3, then the FINAL one waiting for epoch 4; a second stream writes
    the data behind the flag and sets 3, then 4.  What follows the launches in their stream sees the data; the results are those of the
    same chain without a wait."""
    from compactfusion_amd import lanes
    lib, ctx = _lib_ctx()
    a, b = lanes.compute_stream(0), lanes.dedicated_stream(0)          # each owns its hardware queue
    flag = torch.zeros(16, dtype=torch.int32, device="cuda")
    B, S, H, D = 1, 33, 3, 64
    g = torch.Generator(device="cuda").manual_seed(5)
    blocks = [(torch.randn(B, S, H, D, device="cuda", dtype=dtype, generator=g), torch.randn(B, H, S, device="cuda", dtype=torch.float32, generator=g))
              for _ in range(2)]
    out_r, lse_r, _ = _chain(lib, ctx, blocks, dtype, final=False)
    want = out_r.to(dtype)
    out = torch.empty(B, S, H, D, dtype=torch.float32, device="cuda")
    lse = torch.empty(B, S, H, 1, dtype=torch.float32, device="cuda")
    fin = torch.full((B, S, H, D), float("nan"), dtype=dtype, device="cuda")
    payload = torch.zeros(1 << 22, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    e = _elem(dtype) | BSHD
    with torch.cuda.stream(a):
        assert lib.cfx_attn_merge_ex(ctx, out.data_ptr(), lse.data_ptr(), blocks[0][0].data_ptr(), blocks[0][1].data_ptr(), B, S, H, D, e | FIRST,
                                     flag.data_ptr(), 3, None, a.cuda_stream) == 0
        got3 = payload.sum()                     # runs only after the first launch has seen epoch 3
        assert lib.cfx_attn_merge_ex(ctx, out.data_ptr(), lse.data_ptr(), blocks[1][0].data_ptr(), blocks[1][1].data_ptr(), B, S, H, D, e,
                                     flag.data_ptr(), 4, fin.data_ptr(), a.cuda_stream) == 0
        got4 = payload.sum()
    with torch.cuda.stream(b):
        payload.fill_(1)                         # the data behind the flag
        assert lib.cfx_flag_set(ctx, flag.data_ptr(), 3, b.cuda_stream) == 0
        payload.fill_(2)
        assert lib.cfx_flag_set(ctx, flag.data_ptr(), 4, b.cuda_stream) == 0
    torch.cuda.synchronize()
    assert int(got3) >= payload.numel() and int(got4) == 2 * payload.numel()
    assert _same_bits(fin, want) and _same_bits(lse, lse_r)
    assert lib.cfx_gate_errors(ctx) == 0


# ---- 8, 9: compact_fwd -------------------------------------------------------------------------------------------------------------------
WL = 4


def _fake_path():
    sys.path.insert(0, os.path.join(HERE, "fake_rccl"))
    try:
        import build as fake_build
        return fake_build.build()
    finally:
        sys.path.pop(0)
        sys.modules.pop("build", None)


def _compact_fwd_steps(monkeypatch, lane, dtype, check):
    """test_gpu_bf16.py's set-up: compact_fwd (gather schedule), 4 logical ranks looped back, BINARY, 2 layers, 5 steps, the lane off (one
    native op per layer on the caller's stream) or auto (the layer's chain on the exchange lane).  check(s, l, q, k, v, out, lse, info)
    runs after every call; info: what the call did (see below).  Returns the list of steady steps."""
    from compactfusion_amd import _lib, codecs as K, exchange
    from compactfusion_amd.collector import collector
    from compactfusion_amd.compact import attention, ring, main as cm, xlayer
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig
    from compactfusion_amd.prof import Profiler
    lib = _lib.load()
    ctx = K.context(0)
    monkeypatch.setenv("CFX_RING_SCHEDULE", "gather")
    monkeypatch.setenv("CFX_LANE", lane)
    monkeypatch.delenv("CFX_RING_EXCHANGE_STREAM", raising=False)
    monkeypatch.setattr(ring.dist, "get_rank", lambda g=None: 0)
    monkeypatch.setattr(ring.dist, "get_world_size", lambda g=None: WL)
    monkeypatch.setattr(ring.dist, "all_gather_into_tensor",            # WARMUP steps gather the raw shards through torch.distributed
                        lambda recv, send, group=None: recv.view(WL, -1).copy_(send.view(1, -1).expand(WL, -1)))
    if lane == "auto":
        monkeypatch.setenv("CFX_FAKE_RCCL_MODE", "loopback")
        monkeypatch.setenv("CFX_RING_EXCHANGE", "native")
        fake = _fake_path()

        class LoopComm:
            def __init__(self, group, device):
                c = K.context(device)
                assert lib.cfx_rccl_load(fake.encode()) == 0
                uid = ctypes.create_string_buffer(128)
                assert lib.cfx_comm_unique_id(c, uid) == 0
                self.handle = lib.cfx_comm_create(c, uid, WL, 0)
                assert self.handle
        exchange.set_comm_factory(LoopComm)
    else:
        monkeypatch.delenv("CFX_RING_EXCHANGE", raising=False)
        xlayer.set_p2p_loopback(True)
    Profiler.instance().disable()
    collector.init(collector.Collector("/tmp/none", enabled=False))
    ring._xbuf.clear(); ring._steady.clear(); ring._lane_ok.clear()
    # what a call did: whether the steady layer ran it, and how often the Python merge was entered (ring.py binds the name at import)
    ran, merges = [], []
    orig_run, orig_upd = ring._SteadyLayer.run, ring.update_out_and_lse
    monkeypatch.setattr(ring._SteadyLayer, "run", lambda self, *a: (ran.append(self), orig_run(self, *a))[1])
    monkeypatch.setattr(ring, "update_out_and_lse", lambda *a, **kw: (merges.append(1), orig_upd(*a, **kw))[1])
    monkeypatch.setattr(attention, "update_out_and_lse", lambda *a, **kw: (merges.append(1), orig_upd(*a, **kw))[1])
    steady = []
    try:
        L, STEPS = 2, 5
        shape = (1, 64, 8, 64)
        cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: T.WARMUP if s == 0 else T.BINARY, comp_rank=-1,
                                      residual=1, ef=True, fastpath=True))
        g = torch.Generator().manual_seed(3)

        def drift():
            cur = torch.randn(*shape, generator=g)
            seq = []
            for _ in range(STEPS):
                seq.append(cur.to(dtype).contiguous())
                cur = cur + 0.1 * torch.randn(*shape, generator=g)
            return seq
        qs, ks, vs = [drift() for _ in range(L)], [drift() for _ in range(L)], [drift() for _ in range(L)]
        for s in range(STEPS):
            cm.compact_set_step(s)
            n_ran, n_merges, ids30 = 0, 0, 0
            for l in range(L):
                q, k, v = qs[l][s].cuda(), ks[l][s].cuda(), vs[l][s].cuda()
                torch.cuda.synchronize()
                del ran[:], merges[:]
                assert lib.cfx_profile_enable(ctx, 64, 1 << KID_ATTN_MERGE, 1) == 0
                out, lse, _ = ring.compact_fwd(q, k, v, causal=False, mod_idx=l, current_iter=s)
                torch.cuda.synchronize()
                ids, ms = (ctypes.c_int * 64)(), (ctypes.c_float * 64)()
                n = lib.cfx_profile_read(ctx, ids, ms, 64)
                lib.cfx_profile_enable(ctx, 0, 0, 1)
                assert all(ids[i] == KID_ATTN_MERGE for i in range(n))
                info = dict(steady=len(ran) == 1, fast=bool(ran and ran[0]._fast), py_merges=len(merges), merge_launches=n, shape=shape)
                n_ran += len(ran); n_merges += len(merges); ids30 += n
                check(s, l, q, k, v, out, lse, info)
            print(f"lane {lane} step {s}: steady-layer calls {n_ran}/{L}, update_out_and_lse calls {n_merges}, id-30 launches {ids30}")
            if n_ran == L:
                steady.append(s)
                assert n_merges == 0, f"step {s}: the steady step went through update_out_and_lse {n_merges} times"
                assert ids30 == WL * L, f"step {s}: {ids30} merge launches, expected {WL * L}"
        assert lib.cfx_gate_errors(ctx) == 0
        exs = [e for e in ring._xbuf.values() if e.sig is not None]
        assert exs, "no layer was bound to a native exchange"
        if lane == "off":
            assert all(e.xop is not None and e.xop.dtype == dtype for e in exs), "the one-op layer exchange was not taken"
        else:
            assert all(e.plan is not None for e in exs), "the native lane plan was not used"
        assert ring._steady and all(st._fast is True for st in ring._steady.values()), "a steady layer left the lean block loop"
    finally:
        lib.cfx_profile_enable(ctx, 0, 0, 1)
        exchange.set_comm_factory(None)
        cm._drop_kv_exchanges()
        for e in ring._xbuf.values():
            e.close()
        ring._xbuf.clear(); ring._steady.clear(); ring._lane_ok.clear()
        xlayer.set_p2p_loopback(False)
    return steady


def _kv_of_block(cache, l, t, k, v, shape):
    """the K,V block t of the ring order attends to: the rank's own, or the state the cache holds for peer (0 - t) % W"""
    if t == 0:
        return k, v
    return cache.get_base(f"{l}-{(0 - t) % WL}-k").view(shape), cache.get_base(f"{l}-{(0 - t) % WL}-v").view(shape)


@pytest.mark.parametrize("lane", ["off", "auto"])
def test_compact_fwd_bf16_runs_the_lean_block_loop(monkeypatch, lane):
    """bf16 q, k, v: from the third compressed step on (steps 3 and 4 at the latest; the first ones bind the layer) every layer is a steady
    layer on the lean loop - no update_out_and_lse, exactly W x L merge launches a step, none of them followed by a cast.  out is bf16,
    contiguous, and - like lse - within rtol = atol = 2e-3 (the tolerance test_gpu_bf16.py / test_gpu_schedules.py use) of the merge formula
    written out in eager fp32 over the blocks of the K,V the cache holds; the K,V states are the contract's bits."""
    from compactfusion_amd.compact import main as cm
    from compactfusion_amd.compact.attention import block_attention
    N, C = 64, 512
    state = {}
    worst = [0.0, 0.0]

    def check(s, l, q, k, v, out, lse, info):
        shape = info["shape"]
        B, S, H, D = shape
        assert out.dtype == torch.bfloat16 and tuple(out.shape) == shape and out.is_contiguous()
        assert lse.dtype == torch.float32 and tuple(lse.shape) == (B, H, S)
        if info["steady"]:
            assert info["fast"], f"step {s} layer {l}: the steady layer took the generic loop"
        cache = cm.compact_cache()
        for nm, x in (("k", k), ("v", v)):
            xb = bits(x.cpu()).reshape(N, C)
            state[l, nm] = xb.copy() if s == 0 else BC.compress("binary", xb, state[l, nm])[1]
            for r in range(WL):
                stt = cache.get_base(f"{l}-{r}-{nm}")
                assert stt.dtype == torch.bfloat16 and np.array_equal(bits(stt).reshape(N, C), state[l, nm]), (lane, s, l, r, nm)
        ro = rl = None
        for t in range(WL):
            kk, vv = _kv_of_block(cache, l, t, k, v, shape)
            bo, bl = block_attention(q, kk, vv, 0.0, D ** -0.5, causal=False)
            ro, rl = _formula(ro, rl, bo, bl)
        rl = rl.squeeze(-1).transpose(1, 2)
        worst[0] = max(worst[0], float((out.float() - ro).abs().max()))
        worst[1] = max(worst[1], float((lse - rl).abs().max()))
        torch.testing.assert_close(out.float(), ro, rtol=2e-3, atol=2e-3)
        torch.testing.assert_close(lse, rl, rtol=2e-3, atol=2e-3)
    steady = _compact_fwd_steps(monkeypatch, lane, torch.bfloat16, check)
    print(f"lane {lane}: steady steps {steady}; max |out - formula| {worst[0]:.3e}, max |lse - formula| {worst[1]:.3e}")
    assert 3 in steady and 4 in steady, f"steady steps {steady}"


@pytest.mark.parametrize("lane", ["off", "auto"])
def test_compact_fwd_fp16_is_bit_identical_to_the_previous_sequence(monkeypatch, lane):
    """fp16: per layer, the fused SDPA op per block on the cached K,V, the cfx_attn_merge_wait chain - the call the lean loop used before -
    and .to(torch.float16): compact_fwd's out and lse are those bytes, on every step."""
    from compactfusion_amd.compact import main as cm
    lib, ctx = _lib_ctx()
    sdpa = torch.ops.aten._scaled_dot_product_flash_attention

    def check(s, l, q, k, v, out, lse, info):
        shape = info["shape"]
        B, S, H, D = shape
        assert out.dtype == torch.float16 and tuple(out.shape) == shape and out.is_contiguous()
        if info["steady"]:
            assert info["fast"], f"step {s} layer {l}: the steady layer took the generic loop"
        cache = cm.compact_cache()
        o32 = torch.empty(shape, dtype=torch.float32, device="cuda")
        l32 = torch.empty((B, S, H, 1), dtype=torch.float32, device="cuda")
        keep = []
        sh = torch.cuda.current_stream().cuda_stream
        for t in range(WL):
            kk, vv = _kv_of_block(cache, l, t, k, v, shape)
            res = sdpa(q.transpose(1, 2), kk.transpose(1, 2), vv.transpose(1, 2), 0.0, False, False, scale=D ** -0.5)
            keep.append(res)
            assert res[0].transpose(1, 2).is_contiguous() and res[1].is_contiguous() and res[1].dtype == torch.float32
            assert lib.cfx_attn_merge_wait(ctx, o32.data_ptr(), l32.data_ptr(), res[0].data_ptr(), res[1].data_ptr(), B, S, H, D, 1, int(t == 0),
                                           None, 0, sh) == 0, lib.cfx_last_error_string(ctx)
        torch.cuda.synchronize()
        assert _same_bits(out, o32.to(torch.float16)), (lane, s, l, "out")
        assert _same_bits(lse, l32.squeeze(-1).transpose(1, 2)), (lane, s, l, "lse")
    steady = _compact_fwd_steps(monkeypatch, lane, torch.float16, check)
    assert 3 in steady and 4 in steady, f"steady steps {steady}"
