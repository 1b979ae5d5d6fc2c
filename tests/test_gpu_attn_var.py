"""cfx_attn_fwd_blocks_var on the GPU (-m gpu): the attention of the queries over K,V blocks of UNEQUAL length in ONE launch, against the
float64 witness and the derived bound of tests/_attn_var_f64.py on every case of tests/_attn_var_cases.py, fp16 and bf16; bit for bit
against cfx_attn_fwd_blocks where the two walk the same tiles; every query tile; hipGraph replay; every C-ABI refusal; the Python entry;
and compact_fwd with joint tensors on the steady layer (configure(joint="steady")).  Every test fails on a library without the entry
point or a package without the setting."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import _attn_cases as C
import _attn_f64 as W
import _attn_var_cases as VC
import _attn_var_f64 as VW
import bf16_contract as BC

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BF = 0x100
KID_ATTN_MERGE = 30
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
bits = BC.torch_bits
_refs = {}


def _lib_ctx():
    from compactfusion_amd import _lib, codecs as K
    return _lib.load(), K.context(0)


def ref_of(case, dtype):
    """the case's inputs and its witness / bound, computed once and left unchanged"""
    key = (case["id"], dtype)
    if key not in _refs:
        q, ks, vs, scale = VC.build(case, dtype)
        _refs[key] = (q, ks, vs, scale, VW.reference_and_bound(q, ks, vs, scale, dtype))
    return _refs[key]


def _dev(x, dtype):
    t = torch.from_numpy(x).to(TDT[dtype])
    assert torch.equal(t.float(), torch.from_numpy(x))          # (the case's values ARE values of the element type)
    return t.cuda()


def _count(lib, ctx):
    n = ctypes.c_ulonglong(0)
    assert lib.cfx_attn_fwd_launches(ctx, ctypes.byref(n)) == 0
    return n.value


def _outs(q):
    B, Sq, H, D = q.shape
    return (torch.full((B, Sq, H, D), float("nan"), dtype=q.dtype, device="cuda"), torch.full((B, Sq, H), float("nan"), dtype=torch.float32, device="cuda"))


def _var(lib, ctx, q, ks, vs, scale, out=None, lse=None, stream=None):
    """cfx_attn_fwd_blocks_var; every block must be (B, Sk_i, H, D) contiguous: the launch is told nothing else"""
    B, Sq, H, D = q.shape
    n = len(ks)
    assert all(k.is_contiguous() and v.is_contiguous() and k.shape == v.shape and (k.shape[0], k.shape[2], k.shape[3]) == (B, H, D) for k, v in zip(ks, vs))
    if out is None:
        out, lse = _outs(q)
    P = ctypes.c_void_p * n
    sh = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    rc = lib.cfx_attn_fwd_blocks_var(ctx, n, q.data_ptr(), P(*[t.data_ptr() for t in ks]), P(*[t.data_ptr() for t in vs]),
                                     (ctypes.c_int * n)(*[t.shape[1] for t in ks]), B, Sq, H, D, scale, BF if q.dtype == torch.bfloat16 else 0,
                                     out.data_ptr(), lse.data_ptr(), sh)
    assert rc == 0, lib.cfx_last_error_string(ctx)
    return out, lse


def _equal(lib, ctx, q, ks, vs, scale):
    """cfx_attn_fwd_blocks, the existing entry point: blocks of one length"""
    B, Sq, H, D = q.shape
    n = len(ks)
    assert all(k.shape == ks[0].shape and k.is_contiguous() for k in list(ks) + list(vs))
    out, lse = _outs(q)
    P = ctypes.c_void_p * n
    rc = lib.cfx_attn_fwd_blocks(ctx, n, q.data_ptr(), P(*[t.data_ptr() for t in ks]), P(*[t.data_ptr() for t in vs]), B, Sq, ks[0].shape[1], H, D,
                                 scale, BF if q.dtype == torch.bfloat16 else 0, out.data_ptr(), lse.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.cfx_last_error_string(ctx)
    return out, lse


def _same_bits(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    v = torch.int16 if a.element_size() == 2 else torch.int32
    return torch.equal(a.contiguous().view(v), b.contiguous().view(v))


@pytest.mark.parametrize("dtype", list(TDT))
def test_kernel_against_witness_and_bound(dtype):
    """out and lse of EVERY case of tests/_attn_var_cases.py within the derived bound of the float64 witness, each in ONE counted
    launch; a single key returns v's bits.  (One test per element type over all cases - a case is milliseconds of GPU work -; a miss
    names its case.)"""
    lib, ctx = _lib_ctx()
    for case in VC.CASES:
        q, ks, vs, scale, ref = ref_of(case, dtype)
        dq, dks, dvs = _dev(q, dtype), [_dev(k, dtype) for k in ks], [_dev(v, dtype) for v in vs]
        n0 = _count(lib, ctx)
        out, lse = _var(lib, ctx, dq, dks, dvs, scale)
        torch.cuda.synchronize()
        assert _count(lib, ctx) == n0 + 1, case["id"]
        fo, fl = VW.check(out.float().cpu().numpy(), lse.cpu().numpy(), ref, f"cfx_attn_fwd_blocks_var, {case['id']} {dtype}")
        print(f"{case['id']} {dtype}: {fo:.3f} / {fl:.3f} of the bound (out / lse)")
        if case["sks"] == [1]:
            assert _same_bits(out, dvs[0].expand_as(out)), case["id"]
    assert lib.cfx_gate_errors(ctx) == 0


@pytest.mark.parametrize("dtype", list(TDT))
def test_equal_lengths_are_the_equal_length_launch_bit_for_bit(dtype):
    """blocks of ONE length through the new entry point: cfx_attn_fwd_blocks's out and lse, bit for bit (full tiles, tails, one key a
    block, 16 blocks, both head dims, values to +-1e4)"""
    lib, ctx = _lib_ctx()
    picks = [next(c for c in C.CASES if c["kind"] == kind and c["Sk"] == Sk and c["n"] == n)
             for kind, Sk, n in (("gauss", 100, 16), ("gauss", 64, 3), ("gauss", 65, 16), ("peak", 100, 3), ("peak", 1, 8), ("ramp", 65, 8), ("ramp", 63, 2))]
    assert {c["D"] for c in picks} == {64, 128} and {c["B"] for c in picks} == {1, 2}
    for case in picks:
        q, ks, vs, scale = C.build(case, dtype)
        dq, dks, dvs = _dev(q, dtype), [_dev(k, dtype) for k in ks], [_dev(v, dtype) for v in vs]
        o0, l0 = _equal(lib, ctx, dq, dks, dvs, scale)
        o1, l1 = _var(lib, ctx, dq, dks, dvs, scale)
        torch.cuda.synchronize()
        assert _same_bits(o1, o0) and _same_bits(l1, l0), case["id"]
        W.check(o1.float().cpu().numpy(), l1.cpu().numpy(), W.reference_and_bound(q, ks, vs, scale, dtype), case["id"])


@pytest.mark.parametrize("dtype", list(TDT))
@pytest.mark.parametrize("B,D", [(1, 64), (2, 64), (2, 128)])
def test_whole_tiles_are_one_block_of_the_concatenated_keys_bit_for_bit(B, D, dtype):
    """[64, 128, 192]: every block a whole number of tiles - the tile sequence of ONE block of the 384 keys concatenated (per batch)
    through the existing entry point, so the same bits; at B = 2 the three batch strides differ from each other and from the whole's"""
    lib, ctx = _lib_ctx()
    case = dict(B=B, Sq=129, sks=[64, 128, 192], H=2, D=D, kind="gauss", id=f"tiles-b{B}-d{D}")
    q, ks, vs, scale = VC.build(case, dtype)
    dq, dks, dvs = _dev(q, dtype), [_dev(k, dtype) for k in ks], [_dev(v, dtype) for v in vs]
    o1, l1 = _var(lib, ctx, dq, dks, dvs, scale)
    ck, cv = torch.cat(dks, dim=1).contiguous(), torch.cat(dvs, dim=1).contiguous()
    assert tuple(ck.shape) == (B, 384, 2, D)
    o0, l0 = _equal(lib, ctx, dq, [ck], [cv], scale)
    o2, l2 = _var(lib, ctx, dq, [ck], [cv], scale)
    torch.cuda.synchronize()
    assert _same_bits(o1, o0) and _same_bits(l1, l0) and _same_bits(o2, o0) and _same_bits(l2, l0)
    VW.check(o1.float().cpu().numpy(), l1.cpu().numpy(), VW.reference_and_bound(q, ks, vs, scale, dtype), case["id"])


@pytest.mark.parametrize("dtype", list(TDT))
def test_every_query_tile_returns_the_same_bits(dtype):
    """cfx_set_attn_qtile: 64, 128 and 256 query rows a workgroup give the library's choice's bits (D = 64 and 128; Sq = 129: 5 waves)"""
    lib, ctx = _lib_ctx()
    for case in (next(c for c in VC.CASES if c["kind"] == "gauss" and c["sks"] == [100, 37, 128, 5] and c["D"] == 64),
                 next(c for c in VC.CASES if c["kind"] == "gauss" and c["D"] == 128 and c["Sq"] == 129)):
        assert case["Sq"] == 129
        q, ks, vs, scale, ref = ref_of(case, dtype)
        dq, dks, dvs = _dev(q, dtype), [_dev(k, dtype) for k in ks], [_dev(v, dtype) for v in vs]
        out, lse = _var(lib, ctx, dq, dks, dvs, scale)
        try:
            for rows in (64, 128, 256):
                assert lib.cfx_set_attn_qtile(ctx, rows) == 0
                o, l = _var(lib, ctx, dq, dks, dvs, scale)
                torch.cuda.synchronize()
                assert _same_bits(o, out) and _same_bits(l, lse), (case["id"], rows)
        finally:
            assert lib.cfx_set_attn_qtile(ctx, 0) == 0
        VW.check(out.float().cpu().numpy(), lse.cpu().numpy(), ref, "the library's tile")


def test_hipgraph_replay():
    """ONE launch captured over [100, 37, 128, 5] and replayed 3 times, the inputs rewritten in place between replays: every replay
    within the bound (the key counts, like the pointers, are the graph's)"""
    lib, ctx = _lib_ctx()
    base = dict(B=2, Sq=80, sks=[100, 37, 128, 5], H=2, D=64)
    cases = [dict(base, kind=kind, id=f"graph-{i}-{kind}", **kw) for i, (kind, kw) in
             enumerate((("gauss", {}), ("peak", {"pblk": 1, "pend": "last"}), ("ramp", {}), ("peak", {"pblk": 3, "pend": "first"})))]
    q, ks, vs, scale = VC.build(cases[0], "fp16")
    dq, dks, dvs = _dev(q, "fp16"), [_dev(k, "fp16") for k in ks], [_dev(v, "fp16") for v in vs]
    out, lse = _outs(dq)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    n0 = _count(lib, ctx)
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            _var(lib, ctx, dq, dks, dvs, scale, out, lse, side.cuda_stream)
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "capture must not execute"
    assert _count(lib, ctx) == n0 + 1                           # the count is of calls enqueued: replays are the graph's
    for rep, c in enumerate(cases[1:]):
        q2, ks2, vs2, scale2 = VC.build(c, "fp16")
        assert scale2 == scale
        for dst, src in zip([dq] + dks + dvs, [q2] + ks2 + vs2):
            dst.copy_(_dev(src, "fp16"))
        out.fill_(float("nan"))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        fo, fl = VW.check(out.float().cpu().numpy(), lse.cpu().numpy(), VW.reference_and_bound(q2, ks2, vs2, scale, "fp16"), f"replay {rep}")
        print(f"replay {rep} ({c['kind']}): {fo:.3f} / {fl:.3f} of the bound")
    assert rep == 2 and _count(lib, ctx) == n0 + 1 and lib.cfx_gate_errors(ctx) == 0


def test_c_abi_refusals_in_order_launch_nothing():
    """every refusal on live device pointers, in the documented order - NULL, flag, shape / n / key counts / scale, alignment, a tripped
    gate -; each returns before any launch: the count does not move and the outputs keep their NaNs"""
    lib, ctx = _lib_ctx()
    NULL, SHAPE, ALIGN, CODEC, GATE = -1, -2, -3, -4, -8
    B, Sq, H, D = 1, 4, 2, 64
    q = torch.zeros(B, Sq, H, D, dtype=torch.float16, device="cuda")
    kv = [torch.zeros(B, 4 + i, H, D + 8, dtype=torch.float16, device="cuda") for i in range(17)]      # (spare elements: room for a misaligned pointer)
    out = torch.full((B, Sq, H, D + 8), float("nan"), dtype=torch.float16, device="cuda")
    lse = torch.full((B, Sq, H + 4), float("nan"), dtype=torch.float32, device="cuda")
    P, I = ctypes.c_void_p * 17, ctypes.c_int * 17
    ks = P(*[t.data_ptr() for t in kv])
    sk = I(*[4 + i for i in range(17)])
    f = lib.cfx_attn_fwd_blocks_var
    sh = torch.cuda.current_stream().cuda_stream
    n0 = _count(lib, ctx)
    qp, op, lp = q.data_ptr(), out.data_ptr(), lse.data_ptr()
    holed = P(*[None if i == 1 else kv[i].data_ptr() for i in range(17)])
    bad_al = P(*[kv[i].data_ptr() + (2 if i == 1 else 0) for i in range(17)])
    nokeys = I(*[0 if i == 1 else 4 + i for i in range(17)])
    steps = [
        (NULL, (ctx, 2, None, ks, ks, sk, B, Sq, H, D, 0.125, 0x40, op + 2, lp, sh)),          # NULL before the flag, the shape and the alignment
        (NULL, (ctx, 2, qp, holed, ks, sk, B, Sq, H, 20, 0.125, 0x40, op + 2, lp, sh)),
        (NULL, (ctx, 2, qp, ks, holed, sk, B, Sq, H, D, 0.125, 0, op, lp, sh)),
        (NULL, (ctx, 2, qp, ks, ks, None, B, Sq, H, 20, 0.125, 0x40, op + 2, lp, sh)),
        (CODEC, (ctx, 0, qp, ks, ks, nokeys, B, Sq, H, 20, 0.0, 0x40, op + 2, lp, sh)),        # the flag before n, the shape, the scale and the alignment
        (CODEC, (ctx, 2, qp, ks, ks, sk, B, Sq, H, D, 0.125, 1, op, lp, sh)),
        (SHAPE, (ctx, 17, qp, ks, ks, sk, B, Sq, H, D, 0.125, 0, op + 2, lp, sh)),             # n, sizes, key counts, head dim, scale before the alignment
        (SHAPE, (ctx, 0, qp, ks, ks, sk, B, Sq, H, D, 0.125, BF, op + 2, lp, sh)),
        (SHAPE, (ctx, 2, qp, ks, ks, nokeys, B, Sq, H, D, 0.125, 0, op + 2, lp, sh)),
        (SHAPE, (ctx, 2, qp, ks, ks, sk, B, 0, H, D, 0.125, 0, op + 2, lp, sh)),
        (SHAPE, (ctx, 2, qp, ks, ks, sk, B, Sq, H, 96, 0.125, 0, op + 2, lp, sh)),
        (SHAPE, (ctx, 2, qp, ks, ks, sk, B, Sq, H, D, float("nan"), 0, op + 2, lp, sh)),
        (SHAPE, (ctx, 2, qp, ks, ks, sk, B, Sq, H, D, -1.0, 0, op + 2, lp, sh)),
        (ALIGN, (ctx, 2, qp, ks, ks, sk, B, Sq, H, D, 0.125, 0, op + 2, lp, sh)),
        (ALIGN, (ctx, 2, qp, ks, ks, sk, B, Sq, H, D, 0.125, 0, op, lp + 4, sh)),
        (ALIGN, (ctx, 2, qp, bad_al, ks, sk, B, Sq, H, D, 0.125, 0, op, lp, sh)),
        (ALIGN, (ctx, 2, qp, ks, bad_al, sk, B, Sq, H, D, 0.125, BF, op, lp, sh)),
    ]
    for want, a in steps:
        assert f(*a) == want, (want, a[1], a[9:12], lib.cfx_last_error_string(ctx))
    # a tripped gate: a flag wait that times out leaves the context's error word set; the next call is refused - after all the others
    flag = torch.zeros(16, dtype=torch.int32, device="cuda")
    assert lib.cfx_set_gate_timeout_ms(ctx, 1) == 0         # (1 ms: the shortest wait there is)
    try:
        assert lib.cfx_flag_wait(ctx, flag.data_ptr(), 1, sh) == 0
        torch.cuda.synchronize()
        assert f(ctx, 2, qp, ks, ks, sk, B, Sq, H, D, 0.125, 0, op + 2, lp, sh) == ALIGN      # ... the alignment still comes first
        assert f(ctx, 2, qp, ks, ks, sk, B, Sq, H, D, 0.125, 0, op, lp, sh) == GATE
    finally:
        lib.cfx_set_gate_timeout_ms(ctx, 5000)
        assert lib.cfx_gate_recover(ctx) >= 1                   # (the failed waits that were pending; clears the word)
    torch.cuda.synchronize()
    assert _count(lib, ctx) == n0 and torch.isnan(out).all() and torch.isnan(lse).all()
    assert f(ctx, 2, qp, ks, ks, sk, B, Sq, H, D, 0.125, 0, op, lp, sh) == 0 and _count(lib, ctx) == n0 + 1       # the context works again
    torch.cuda.synchronize()


def test_python_entry_takes_the_launch_on_unequal_blocks():
    """attention_blocks on GPU blocks that differ in their key count is ONE launch, proved by the counter (before: the eager definition);
    equal blocks keep theirs; what neither launch takes runs the eager definition; more than 16 blocks are refused"""
    from compactfusion_amd.compact import attention as A
    lib, ctx = _lib_ctx()
    case = next(c for c in VC.CASES if c["kind"] == "gauss" and c["sks"] == [130, 40, 40] and c["D"] == 64)
    for dtype in TDT:
        q, ks, vs, scale, ref = ref_of(case, dtype)
        dq, dks, dvs = _dev(q, dtype), [_dev(k, dtype) for k in ks], [_dev(v, dtype) for v in vs]
        assert A.attn_native_var_ok(dq, dks, dvs) and not A.attn_native_ok(dq, dks, dvs)
        n0 = A.attn_fwd_launches(0)
        out, lse = A.attention_blocks(dq, dks, dvs)             # the default scale: D ** -0.5
        torch.cuda.synchronize()
        assert A.attn_fwd_launches(0) == n0 + 1
        B, Sq, H, D = q.shape
        assert out.dtype == TDT[dtype] and out.is_contiguous() and tuple(lse.shape) == (B, H, Sq) and lse.stride() == (Sq * H, 1, H)
        VW.check(out.float().cpu().numpy(), lse.transpose(1, 2).cpu().numpy(), ref, "attention_blocks")
        o1, l1 = _var(lib, ctx, dq, dks, dvs, scale)
        assert _same_bits(out, o1) and _same_bits(lse.transpose(1, 2), l1)
        n1 = A.attn_fwd_launches(0)
        # one block non-contiguous, K and V of a block of different lengths, fp32: the eager definition, no launch
        odd = [dks[0].transpose(1, 2).contiguous().transpose(1, 2)] + dks[1:]
        assert not A.attn_native_var_ok(dq, odd, dvs) and not A.attn_native_var_ok(dq, dks, [dvs[0][:, :100].contiguous()] + dvs[1:])
        o2, l2 = A.attention_blocks(dq, odd, dvs, scale)
        o3, _ = A.attention_blocks(dq.float(), [k.float() for k in dks], [v.float() for v in dvs], scale)
        assert A.attn_fwd_launches(0) == n1 and o3.dtype == torch.float32
        VW.check(o2.float().cpu().numpy(), l2.transpose(1, 2).cpu().numpy(), ref, "attention_blocks, eager on the GPU")
        with pytest.raises(ValueError, match="at most 16"):
            A.attention_blocks(dq, dks * 6, dvs * 6, scale)
        assert A.attn_fwd_launches(0) == n1
        A.attention_blocks(dq, dks[1:], dvs[1:], scale)         # equal blocks: the equal-length launch, as before
        assert A.attn_fwd_launches(0) == n1 + 1


# ---- compact_fwd with joint tensors on the steady layer ----------------------------------------------------------------------------------
WL, L, STEPS, PLAIN = 4, 2, 5, 4             # ranks, layers, the last step, the one step WITHOUT joint tensors
KV, QS, JS = (1, 64, 8, 64), (1, 80, 8, 64), (1, 16, 8, 64)
_runs = {}


def _fake_path():
    sys.path.insert(0, os.path.join(HERE, "fake_rccl"))
    try:
        import build as fake_build
        return fake_build.build()
    finally:
        sys.path.pop(0)
        sys.modules.pop("build", None)


def _run_steps(monkeypatch, lane, dtype, strategy, joint, attention="sdpa", merge="chain"):
    """L layers x STEPS + 1 steps of compact_fwd, 4 logical ranks looped back, 1-bit codec (the loop-back harness of
    tests/test_gpu_attn_fwd.py), K,V (1, 64, 8, 64), q (1, 80, 8, 64) and - on every step but PLAIN - joint tensors (1, 16, 8, 64) with
    `strategy`, under configure(joint=joint, attention=attention, attn_merge=merge).  Per (step, layer): out, lse, the K,V states of every
    rank, whether the steady layer ran, the attention launches by the context's counter, the fused SDPA calls, the id-30 merge launches
    and the stand-alone cfx_flag_wait calls on the layer's own "peer s reconstructed" flags."""
    from compactfusion_amd import _lib, codecs as K, config, exchange
    from compactfusion_amd.collector import collector
    from compactfusion_amd.compact import ring, main as cm, xlayer
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig
    from compactfusion_amd.prof import Profiler
    lib = _lib.load()
    ctx = K.context(0)
    config.reset()
    monkeypatch.setenv("CFX_ATTENTION", attention)
    monkeypatch.setenv("CFX_ATTN_MERGE", merge)
    if joint is None:
        monkeypatch.delenv("CFX_JOINT", raising=False)
    else:
        monkeypatch.setenv("CFX_JOINT", joint)
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
    ran, waits, sdpas = [], [], []
    orig_run, orig_wait = ring._SteadyLayer.run, lib.cfx_flag_wait
    orig_sdpa = torch.ops.aten._scaled_dot_product_flash_attention
    monkeypatch.setattr(ring._SteadyLayer, "run", lambda self, *a: (ran.append(self), orig_run(self, *a))[1])
    monkeypatch.setattr(lib, "cfx_flag_wait", lambda *a: (waits.append(a), orig_wait(*a))[1])
    monkeypatch.setattr(torch.ops.aten, "_scaled_dot_product_flash_attention", lambda *a, **kw: (sdpas.append(1), orig_sdpa(*a, **kw))[1])
    rows = {}
    try:
        dname = "fp16" if dtype == torch.float16 else "bf16"
        cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: T.WARMUP if s == 0 else T.BINARY, comp_rank=-1,
                                      residual=1, ef=True, fastpath=True))
        g = torch.Generator().manual_seed(5)

        def drift(shape):
            cur = torch.randn(*shape, generator=g)
            seq = []
            for _ in range(STEPS + 1):
                seq.append(cur.to(dtype).contiguous())
                cur = cur + 0.1 * torch.randn(*shape, generator=g)
            return seq
        qs, ks, vs = [drift(QS) for _ in range(L)], [drift(KV) for _ in range(L)], [drift(KV) for _ in range(L)]
        jks, jvs = [drift(JS) for _ in range(L)], [drift(JS) for _ in range(L)]
        for s in range(STEPS + 1):
            cm.compact_set_step(s)
            for l in range(L):
                q, k, v, jk, jv = (t[l][s].cuda() for t in (qs, ks, vs, jks, jvs))
                joint_kw = dict(joint_tensor_key=jk, joint_tensor_value=jv, joint_strategy=strategy) if s != PLAIN else {}
                torch.cuda.synchronize()
                del ran[:], waits[:], sdpas[:]
                n0 = _count(lib, ctx)
                assert lib.cfx_profile_enable(ctx, 64, 1 << KID_ATTN_MERGE, 1) == 0
                out, lse, _ = ring.compact_fwd(q, k, v, causal=False, mod_idx=l, current_iter=s, **joint_kw)
                torch.cuda.synchronize()
                ids, ms = (ctypes.c_int * 64)(), (ctypes.c_float * 64)()
                merges = lib.cfx_profile_read(ctx, ids, ms, 64)
                lib.cfx_profile_enable(ctx, 0, 0, 1)
                n1 = _count(lib, ctx)
                steady = len(ran) == 1
                assert out.dtype == dtype and tuple(out.shape) == QS and out.is_contiguous()
                assert lse.dtype == torch.float32 and tuple(lse.shape) == (QS[0], QS[2], QS[1])
                cache = cm.compact_cache()
                states = {(r, nm): bits(cache.get_base(f"{l}-{r}-{nm}")).copy() for r in range(WL) for nm in ("k", "v")}
                # the stand-alone waits on the layer's own peer flags (the hand-over to and from the lane waits on other words)
                st = ring._steady.get((l, None))
                peer_flags = [st.ex.flag_ptr(t) for t in range(1, WL)] if st is not None and st.ex.plan is not None else []
                n_waits = sorted(peer_flags.index(a[1]) for a in waits if a[1] in peer_flags)
                # the float64 witness over the K,V the rank holds: [joint ;] own, the peers' reconstructed states in ring order [; joint]
                kk = [k] + [cache.get_base(f"{l}-{(0 - t) % WL}-k").view(KV) for t in range(1, WL)]
                vv = [v] + [cache.get_base(f"{l}-{(0 - t) % WL}-v").view(KV) for t in range(1, WL)]
                if joint_kw:
                    kk, vv = ([jk] + kk, [jv] + vv) if strategy == "front" else (kk + [jk], vv + [jv])
                ref = VW.reference_and_bound(q.float().cpu().numpy(), [t.float().cpu().numpy() for t in kk], [t.float().cpu().numpy() for t in vv],
                                             QS[-1] ** -0.5, dname)
                if attention == "native" and steady:             # the one launch: held to ITS bound; the sdpa forms to the tolerance their own test uses
                    fo, fl = VW.check(out.float().cpu().numpy(), lse.transpose(1, 2).cpu().numpy(), ref, f"compact_fwd native {s, l}")
                    print(f"step {s} layer {l} joint {bool(joint_kw)}: {fo:.3f} / {fl:.3f} of the bound")
                else:
                    torch.testing.assert_close(out.float().cpu(), torch.from_numpy(ref[0]).float(), rtol=2e-3, atol=2e-3 if dtype == torch.float16 else 1.6e-2)
                    torch.testing.assert_close(lse.transpose(1, 2).cpu(), torch.from_numpy(ref[1]).float(), rtol=2e-3, atol=2e-3)
                rows[s, l] = dict(out=out.clone(), lse=lse.clone(), lse_stride=lse.stride(), states=states, steady=steady, joint=bool(joint_kw),
                                  attn=n1 - n0, sdpa=len(sdpas), merges=merges, waits=n_waits)
        assert lib.cfx_gate_errors(ctx) == 0
        exs = [e for e in ring._xbuf.values() if e.sig is not None]
        assert exs, "no layer was bound to a native exchange"
        if lane == "off":
            assert all(e.xop is not None for e in exs), "the one-op layer exchange was not taken"
        else:
            assert all(e.plan is not None for e in exs), "the native lane plan was not used"
    finally:
        lib.cfx_profile_enable(ctx, 0, 0, 1)
        exchange.set_comm_factory(None)
        cm._drop_kv_exchanges()
        for e in ring._xbuf.values():
            e.close()
        ring._xbuf.clear(); ring._steady.clear(); ring._lane_ok.clear()
        xlayer.set_p2p_loopback(False)
        config.reset()
    return rows


def _general(monkeypatch, lane, dtype, strategy):
    """the same seeded sequence with `joint` left unset (the default, "general"): run once per (lane, dtype, strategy), left unchanged"""
    key = (lane, dtype, strategy)
    if key not in _runs:
        _runs[key] = _run_steps(monkeypatch, lane, dtype, strategy, None)
    return _runs[key]


# joint="steady" x lane x strategy x attention, fp16; bf16 on the native rows; attn_merge="once" on one sdpa row per lane
GRID = [(lane, strategy, a, "chain", d) for lane in ("off", "auto") for strategy in ("front", "rear")
        for a, d in (("sdpa", "fp16"), ("native", "fp16"), ("native", "bf16"))] + [("off", "front", "sdpa", "once", "fp16"), ("auto", "rear", "sdpa", "once", "fp16")]


@pytest.mark.parametrize("lane,strategy,attention,merge,dname", GRID, ids=["-".join(g) for g in GRID])
def test_compact_fwd_joint_on_the_steady_layer(monkeypatch, lane, strategy, attention, merge, dname):
    """configure(joint="steady") against the same seeded sequence with `joint` unset: the K,V states of every rank bit-identical call for
    call; once bound the steady layer runs on the joint calls AND on the call without joint tensors between them; unset, no joint call
    runs it.  native: per steady call exactly ONE attention launch, no SDPA call, no merge launch, on the lane one stand-alone wait on
    each of the W-1 peer flags, out / lse within the witness's bound over [joint ; own ; peers] in the strategy's order (in _run_steps).
    sdpa: W SDPA calls (+1 for the lean loop's trial), W merges (chain) or ONE (once), out / lse against the general run."""
    dtype = TDT[dname]
    gen = _general(monkeypatch, lane, dtype, strategy)
    got = _run_steps(monkeypatch, lane, dtype, strategy, "steady", attention, merge)
    assert gen.keys() == got.keys() and any(v["joint"] for v in gen.values())
    rt, at = 2e-3, 2e-3 if dtype == torch.float16 else 1.6e-2
    steady = []
    for key in sorted(gen):
        a, b = gen[key], got[key]
        for sk in a["states"]:
            assert np.array_equal(a["states"][sk], b["states"][sk]), (key, sk)
        assert a["joint"] == b["joint"] == (key[0] != PLAIN)
        assert not (a["joint"] and a["steady"]), f"{key}: with `joint` unset a call with joint tensors ran the steady layer"
        assert a["attn"] == 0 and a["lse_stride"] == b["lse_stride"] and a["out"].stride() == b["out"].stride()
        if not a["joint"]:
            assert a["steady"] == b["steady"]
        if not b["steady"]:                                      # the binding calls: today's path, call for call
            assert b["attn"] == 0 and b["sdpa"] == a["sdpa"] > 0 and b["merges"] == a["merges"], (key, a["sdpa"], b["sdpa"], a["merges"], b["merges"])
            assert _same_bits(a["out"], b["out"]) and _same_bits(a["lse"].contiguous(), b["lse"].contiguous()), key
            continue
        steady.append(key)
        if attention == "native":
            assert b["attn"] == 1 and b["sdpa"] == 0 and b["merges"] == 0, f"{key}: native made {b['attn']} launches, {b['sdpa']} SDPA calls, {b['merges']} merges"
            assert b["waits"] == (list(range(WL - 1)) if lane == "auto" else []), f"{key}: stand-alone waits on peer flags {b['waits']}"
        else:
            assert b["attn"] == 0 and b["sdpa"] in (WL, WL + 1) and b["merges"] == (1 if merge == "once" else WL), \
                f"{key}: the sdpa form made {b['attn']} launches, {b['sdpa']} SDPA calls, {b['merges']} merges"
            torch.testing.assert_close(b["out"].float(), a["out"].float(), rtol=rt, atol=at)
            torch.testing.assert_close(b["lse"], a["lse"], rtol=2e-3, atol=2e-3)
    print(f"lane {lane} {strategy} {attention} {merge} {dname}: steady (step, layer) {steady}")
    assert {(s, l) for s in (3, 4, 5) for l in range(L)} <= set(steady), steady      # joint (3, 5) and plain (4) calls on one steady layer
