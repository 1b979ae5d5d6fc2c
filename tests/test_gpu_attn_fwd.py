"""cfx_attn_fwd_blocks on the GPU (-m gpu): the attention of the queries over all K,V blocks in ONE launch, against the float64 witness and
the derived bound of tests/_attn_f64.py on every case of tests/_attn_cases.py, fp16 and bf16; the single key bit for bit; the FLUX
shape; scattered blocks, table order and allocation order; hipGraph replay; every C-ABI refusal; the Python entry; and compact_fwd with
configure(attention="native").  Every test fails on a library without the entry point."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import _attn_cases as C
import _attn_f64 as W
import bf16_contract as BC

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BF = 0x100
KID_ATTN_MERGE = 30
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
IDS = [c["id"] for c in C.CASES]
bits = BC.torch_bits
_refs = {}


@pytest.fixture(autouse=True)
def _collector(tmp_path):
    from compactfusion_amd.collector import collector
    collector.init(collector.Collector(str(tmp_path), enabled=False))
    yield


def _lib_ctx():
    from compactfusion_amd import _lib, codecs as K
    return _lib.load(), K.context(0)


def ref_of(case, dtype):
    """the case's inputs and its witness / bound, computed once and left unchanged"""
    key = (case["id"], dtype)
    if key not in _refs:
        q, ks, vs, scale = C.build(case, dtype)
        _refs[key] = (q, ks, vs, scale, W.reference_and_bound(q, ks, vs, scale, dtype))
    return _refs[key]


def _dev(x, dtype):
    t = torch.from_numpy(x).to(TDT[dtype]).cuda()
    assert torch.equal(t.float().cpu(), torch.from_numpy(x))
    return t


def _count(lib, ctx):
    n = ctypes.c_ulonglong(0)
    assert lib.cfx_attn_fwd_launches(ctx, ctypes.byref(n)) == 0
    return n.value


def _fwd(lib, ctx, q, ks, vs, scale, out=None, lse=None, stream=None):
    B, Sq, H, D = q.shape
    n = len(ks)
    if out is None:
        out = torch.full((B, Sq, H, D), float("nan"), dtype=q.dtype, device="cuda")
        lse = torch.full((B, Sq, H), float("nan"), dtype=torch.float32, device="cuda")
    P = ctypes.c_void_p * n
    sh = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    rc = lib.cfx_attn_fwd_blocks(ctx, n, q.data_ptr(), P(*[t.data_ptr() for t in ks]), P(*[t.data_ptr() for t in vs]), B, Sq, ks[0].shape[1], H, D,
                                 scale, BF if q.dtype == torch.bfloat16 else 0, out.data_ptr(), lse.data_ptr(), sh)
    assert rc == 0, lib.cfx_last_error_string(ctx)
    return out, lse


def _same_bits(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    v = torch.int16 if a.element_size() == 2 else torch.int32
    return torch.equal(a.contiguous().view(v), b.contiguous().view(v))


def _check_case(case, dtype):
    lib, ctx = _lib_ctx()
    q, ks, vs, scale, ref = ref_of(case, dtype)
    dq, dks, dvs = _dev(q, dtype), [_dev(k, dtype) for k in ks], [_dev(v, dtype) for v in vs]
    n0 = _count(lib, ctx)
    out, lse = _fwd(lib, ctx, dq, dks, dvs, scale)
    torch.cuda.synchronize()
    assert _count(lib, ctx) == n0 + 1
    fo, fl = W.check(out.float().cpu().numpy(), lse.cpu().numpy(), ref, "cfx_attn_fwd_blocks")
    print(f"{case['id']} {dtype}: {fo:.3f} / {fl:.3f} of the bound (out / lse)")
    if case["n"] == 1 and case["Sk"] == 1:                     # the single key: out is v's bits, lse the fp32 product (q . k) * scale
        assert _same_bits(out, dvs[0].expand_as(out))
        if case["kind"] == "int":                              # (integer q, k: the fp32 sum is exact in any order)
            dot = np.einsum("bqhd,bkhd->bqh", q.astype(np.float64), ks[0].astype(np.float64)).astype(np.float32)
            assert np.array_equal(lse.cpu().numpy(), dot * np.float32(scale))
    assert lib.cfx_gate_errors(ctx) == 0
    return dq, dks, dvs, scale, out, lse


@pytest.mark.parametrize("dtype", list(TDT))
@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_kernel_against_witness_and_bound(case, dtype):
    """out and lse of every case within the derived bound of the float64 witness, in ONE counted launch; n = 1, Sk = 1 bit for bit"""
    _check_case(case, dtype)


def test_flux_shape():
    """(1, 544, 24, 128), 8 blocks of 544 keys, bf16: the shard compact_fwd attends over on FLUX"""
    _check_case(C.FLUX, "bf16")


@pytest.mark.parametrize("dtype", list(TDT))
def test_scattered_blocks_table_order_and_allocation_order(dtype):
    """blocks at scattered addresses (separate allocations with gaps between them) - and the same bits when the same blocks sit in ONE
    buffer, and when they were allocated in the reverse order (the table, not the address, orders the walk)"""
    lib, ctx = _lib_ctx()
    case = next(c for c in C.CASES if c["kind"] == "gauss" and c["n"] == 8)
    q, ks, vs, scale, ref = ref_of(case, dtype)
    dq = _dev(q, dtype)
    gaps, dks, dvs = [], [], []
    for i, (k, v) in enumerate(zip(ks, vs)):                    # separate allocations, odd-sized gaps between them
        dks.append(_dev(k, dtype)); gaps.append(torch.empty(4096 * (i + 1) + 16, dtype=torch.uint8, device="cuda")); dvs.append(_dev(v, dtype))
    ptrs = [t.data_ptr() for t in dks + dvs]
    assert len(set(ptrs)) == len(ptrs) and any(b - a != dks[0].numel() * 2 for a, b in zip(sorted(ptrs), sorted(ptrs)[1:]))
    out, lse = _fwd(lib, ctx, dq, dks, dvs, scale)
    W.check(out.float().cpu().numpy(), lse.cpu().numpy(), ref, "scattered blocks")
    one_k, one_v = torch.stack(dks), torch.stack(dvs)           # ONE buffer each
    o1, l1 = _fwd(lib, ctx, dq, list(one_k.unbind(0)), list(one_v.unbind(0)), scale)
    rk = [_dev(k, dtype) for k in reversed(ks)][::-1]           # allocated last block first
    rv = [_dev(v, dtype) for v in reversed(vs)][::-1]
    o2, l2 = _fwd(lib, ctx, dq, rk, rv, scale)
    torch.cuda.synchronize()
    assert _same_bits(o1, out) and _same_bits(l1, lse) and _same_bits(o2, out) and _same_bits(l2, lse)


@pytest.mark.parametrize("dtype", list(TDT))
def test_every_query_tile_returns_the_same_bits(dtype):
    """cfx_set_attn_qtile: 64, 128 and 256 query rows a workgroup - a wave's 32 rows walk the same tiles in the same order whatever the
    workgroup around it, so the results are the library's choice's, bit for bit (D = 128 and D = 64; Sq = 257 and 130: 9 and 5 waves)"""
    lib, ctx = _lib_ctx()
    for case in (next(c for c in C.CASES if c["Sq"] == 257 and c["D"] == 128), next(c for c in C.CASES if c["Sq"] == 130 and c["D"] == 64)):
        q, ks, vs, scale, ref = ref_of(case, dtype)
        dq, dks, dvs = _dev(q, dtype), [_dev(k, dtype) for k in ks], [_dev(v, dtype) for v in vs]
        out, lse = _fwd(lib, ctx, dq, dks, dvs, scale)
        try:
            for rows in (64, 128, 256):
                assert lib.cfx_set_attn_qtile(ctx, rows) == 0
                o, l = _fwd(lib, ctx, dq, dks, dvs, scale)
                torch.cuda.synchronize()
                assert _same_bits(o, out) and _same_bits(l, lse), (case["id"], rows)
            assert lib.cfx_set_attn_qtile(ctx, 96) == -2
        finally:
            assert lib.cfx_set_attn_qtile(ctx, 0) == 0
        W.check(out.float().cpu().numpy(), lse.cpu().numpy(), ref, "the library's tile")


def test_hipgraph_replay():
    """the launch captured at n = 8 and replayed 3 times, the inputs rewritten in place between replays: every replay within the bound"""
    lib, ctx = _lib_ctx()
    base = dict(B=1, Sq=65, Sk=100, n=8, H=3, D=128)
    cases = [dict(base, kind=kind, id=f"graph-{kind}", **kw) for kind, kw in (("gauss", {}), ("peak", {"where": "tail"}), ("ramp", {}), ("vmax", {}))]
    q, ks, vs, scale = C.build(cases[0], "fp16")
    dq, dks, dvs = _dev(q, "fp16"), [_dev(k, "fp16") for k in ks], [_dev(v, "fp16") for v in vs]
    out = torch.full(q.shape, float("nan"), dtype=torch.float16, device="cuda")
    lse = torch.full(q.shape[:3], float("nan"), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    n0 = _count(lib, ctx)
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            _fwd(lib, ctx, dq, dks, dvs, scale, out, lse, side.cuda_stream)
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "capture must not execute"
    assert _count(lib, ctx) == n0 + 1                           # the count is of calls enqueued: replays are the graph's
    for rep, c in enumerate(cases[1:]):
        q2, ks2, vs2, scale2 = C.build(c, "fp16")
        assert scale2 == scale
        for dst, src in zip([dq] + dks + dvs, [q2] + ks2 + vs2):
            dst.copy_(_dev(src, "fp16"))
        out.fill_(float("nan"))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        fo, fl = W.check(out.float().cpu().numpy(), lse.cpu().numpy(), W.reference_and_bound(q2, ks2, vs2, scale, "fp16"), f"replay {rep}")
        print(f"replay {rep} ({c['kind']}): {fo:.3f} / {fl:.3f} of the bound")
    assert lib.cfx_gate_errors(ctx) == 0


def test_c_abi_refusals_in_order_launch_nothing():
    """every refusal on live device pointers, in the documented order - NULL, flag, shape / n / scale, alignment, a tripped gate -; each
    returns before any launch: the count does not move and the outputs keep their NaNs"""
    from compactfusion_amd import _lib
    lib, ctx = _lib_ctx()
    NULL, SHAPE, ALIGN, CODEC, GATE = -1, -2, -3, -4, -8
    B, Sq, Sk, H, D = 1, 4, 4, 2, 64
    q = torch.zeros(B, Sq, H, D, dtype=torch.float16, device="cuda")
    kv = [torch.zeros(B, Sk, H, D + 8, dtype=torch.float16, device="cuda") for _ in range(17)]      # (8 spare elements: room for a misaligned pointer)
    out = torch.full((B, Sq, H, D + 8), float("nan"), dtype=torch.float16, device="cuda")
    lse = torch.full((B, Sq, H + 4), float("nan"), dtype=torch.float32, device="cuda")
    P = ctypes.c_void_p * 17
    ks = P(*[t.data_ptr() for t in kv])
    f = lib.cfx_attn_fwd_blocks
    sh = torch.cuda.current_stream().cuda_stream
    n0 = _count(lib, ctx)
    qp, op, lp = q.data_ptr(), out.data_ptr(), lse.data_ptr()
    holed = P(*[None if i == 1 else kv[i].data_ptr() for i in range(17)])
    bad_al = P(*[kv[i].data_ptr() + (2 if i == 1 else 0) for i in range(17)])
    steps = [
        (NULL, (ctx, 2, None, ks, ks, B, Sq, Sk, H, D, 0.125, 0x40, op + 2, lp, sh)),          # NULL before the flag, the shape and the alignment
        (NULL, (ctx, 2, qp, holed, ks, B, Sq, Sk, H, 20, 0.125, 0x40, op + 2, lp, sh)),
        (NULL, (ctx, 2, qp, ks, holed, B, Sq, Sk, H, D, 0.125, 0, op, lp, sh)),
        (CODEC, (ctx, 0, qp, ks, ks, B, Sq, Sk, H, 20, 0.0, 0x40, op + 2, lp, sh)),            # the flag before n, the shape, the scale and the alignment
        (CODEC, (ctx, 2, qp, ks, ks, B, Sq, Sk, H, D, 0.125, 1, op, lp, sh)),
        (SHAPE, (ctx, 17, qp, ks, ks, B, Sq, Sk, H, D, 0.125, 0, op + 2, lp, sh)),             # n, sizes, head dim, scale before the alignment
        (SHAPE, (ctx, 0, qp, ks, ks, B, Sq, Sk, H, D, 0.125, BF, op + 2, lp, sh)),
        (SHAPE, (ctx, 2, qp, ks, ks, B, Sq, 0, H, D, 0.125, 0, op + 2, lp, sh)),
        (SHAPE, (ctx, 2, qp, ks, ks, B, Sq, Sk, H, 96, 0.125, 0, op + 2, lp, sh)),
        (SHAPE, (ctx, 2, qp, ks, ks, B, Sq, Sk, H, D, float("nan"), 0, op + 2, lp, sh)),
        (SHAPE, (ctx, 2, qp, ks, ks, B, Sq, Sk, H, D, -1.0, 0, op + 2, lp, sh)),
        (ALIGN, (ctx, 2, qp, ks, ks, B, Sq, Sk, H, D, 0.125, 0, op + 2, lp, sh)),
        (ALIGN, (ctx, 2, qp, ks, ks, B, Sq, Sk, H, D, 0.125, 0, op, lp + 4, sh)),
        (ALIGN, (ctx, 2, qp, bad_al, ks, B, Sq, Sk, H, D, 0.125, 0, op, lp, sh)),
        (ALIGN, (ctx, 2, qp, ks, bad_al, B, Sq, Sk, H, D, 0.125, BF, op, lp, sh)),
    ]
    for want, a in steps:
        assert f(*a) == want, (want, a[1], a[9:12], lib.cfx_last_error_string(ctx))
    # a tripped gate: a flag wait that times out leaves the context's error word set; the next call is refused - after all the others
    flag = torch.zeros(16, dtype=torch.int32, device="cuda")
    assert lib.cfx_set_gate_timeout_ms(ctx, 1) == 0         # (1 ms: the shortest wait there is)
    try:
        assert lib.cfx_flag_wait(ctx, flag.data_ptr(), 1, sh) == 0
        torch.cuda.synchronize()
        assert f(ctx, 2, qp, ks, ks, B, Sq, Sk, H, D, 0.125, 0, op + 2, lp, sh) == ALIGN      # ... the alignment still comes first
        assert f(ctx, 2, qp, ks, ks, B, Sq, Sk, H, D, 0.125, 0, op, lp, sh) == GATE
    finally:
        lib.cfx_set_gate_timeout_ms(ctx, 5000)
        assert lib.cfx_gate_recover(ctx) >= 1                   # (the failed waits that were pending; clears the word)
    torch.cuda.synchronize()
    assert _count(lib, ctx) == n0 and torch.isnan(out).all() and torch.isnan(lse).all()
    assert f(ctx, 2, qp, ks, ks, B, Sq, Sk, H, D, 0.125, 0, op, lp, sh) == 0 and _count(lib, ctx) == n0 + 1       # the context works again


def test_python_entry_takes_the_native_launch():
    """attention_blocks on GPU tensors is the one launch, proved by the counter; what the launch does not take runs the eager
    definition; more than 16 blocks are refused"""
    from compactfusion_amd.compact import attention as A
    lib, ctx = _lib_ctx()
    case = next(c for c in C.CASES if c["kind"] == "gauss" and c["n"] == 3 and c["D"] == 64)
    for dtype in TDT:
        q, ks, vs, scale, ref = ref_of(case, dtype)
        dq, dks, dvs = _dev(q, dtype), [_dev(k, dtype) for k in ks], [_dev(v, dtype) for v in vs]
        n0 = A.attn_fwd_launches(0)
        assert n0 == _count(lib, ctx)
        out, lse = A.attention_blocks(dq, dks, dvs)             # the default scale: D ** -0.5
        torch.cuda.synchronize()
        assert A.attn_fwd_launches(0) == n0 + 1
        B, Sq, H, D = q.shape
        assert out.dtype == TDT[dtype] and out.is_contiguous() and tuple(lse.shape) == (B, H, Sq) and lse.stride() == (Sq * H, 1, H)
        W.check(out.float().cpu().numpy(), lse.transpose(1, 2).cpu().numpy(), ref, "attention_blocks")
        # a non-contiguous q, fp32 tensors: the eager definition, no launch
        o2, l2 = A.attention_blocks(dq.transpose(1, 2).contiguous().transpose(1, 2), dks, dvs, scale) if Sq > 1 and H > 1 else (out, lse)
        o3, l3 = A.attention_blocks(dq.float(), [k.float() for k in dks], [v.float() for v in dvs], scale)
        assert A.attn_fwd_launches(0) == n0 + 1 and o3.dtype == torch.float32
        W.check(o2.float().cpu().numpy(), l2.transpose(1, 2).cpu().numpy(), ref, "attention_blocks, eager on the GPU")
        with pytest.raises(ValueError, match="at most 16"):
            A.attention_blocks(dq, dks * 6, dvs * 6, scale)
        assert A.attn_fwd_launches(0) == n0 + 1


# ---- compact_fwd with configure(attention="native") ------------------------------------------------------------------------------------
WL = 4


def _fake_path():
    sys.path.insert(0, os.path.join(HERE, "fake_rccl"))
    try:
        import build as fake_build
        return fake_build.build()
    finally:
        sys.path.pop(0)
        sys.modules.pop("build", None)


def _run_steps(monkeypatch, lane, dtype, mode):
    """L layers x STEPS steps of compact_fwd, 4 logical ranks looped back, 1-bit codec, configure(attention=mode) (the loop-back harness of
    tests/test_gpu_attn_merge_many.py).  Per (step, layer): out, lse, the K,V states of every rank, whether the steady layer ran, the
    attention launches by the context's counter, the fused SDPA calls, the id-30 merge launches and the cfx_flag_wait calls - and, after
    the last step, one more call per layer WITH joint tensors."""
    from compactfusion_amd import _lib, codecs as K, config, exchange
    from compactfusion_amd.collector import collector
    from compactfusion_amd.compact import ring, main as cm, xlayer
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig
    from compactfusion_amd.prof import Profiler
    lib = _lib.load()
    ctx = K.context(0)
    config.reset()
    monkeypatch.setenv("CFX_ATTENTION", mode)
    monkeypatch.delenv("CFX_ATTN_MERGE", raising=False)
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
        L, STEPS = 2, 5
        shape = (1, 64, 8, 64)
        dname = "fp16" if dtype == torch.float16 else "bf16"
        cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: T.WARMUP if s == 0 else T.BINARY, comp_rank=-1,
                                      residual=1, ef=True, fastpath=True))
        g = torch.Generator().manual_seed(3)

        def drift():
            cur = torch.randn(*shape, generator=g)
            seq = []
            for _ in range(STEPS + 1):
                seq.append(cur.to(dtype).contiguous())
                cur = cur + 0.1 * torch.randn(*shape, generator=g)
            return seq
        qs, ks, vs = [drift() for _ in range(L)], [drift() for _ in range(L)], [drift() for _ in range(L)]
        jk, jv = torch.randn(1, 16, 8, 64, generator=g).to(dtype).cuda(), torch.randn(1, 16, 8, 64, generator=g).to(dtype).cuda()
        for s in range(STEPS + 1):
            cm.compact_set_step(s)
            for l in range(L):
                q, k, v = qs[l][s].cuda(), ks[l][s].cuda(), vs[l][s].cuda()
                joint = dict(joint_tensor_key=jk, joint_tensor_value=jv, joint_strategy="front") if s == STEPS else {}
                torch.cuda.synchronize()
                del ran[:], waits[:], sdpas[:]
                n0 = ctypes.c_ulonglong(0)
                assert lib.cfx_attn_fwd_launches(ctx, ctypes.byref(n0)) == 0
                assert lib.cfx_profile_enable(ctx, 64, 1 << KID_ATTN_MERGE, 1) == 0
                out, lse, _ = ring.compact_fwd(q, k, v, causal=False, mod_idx=l, current_iter=s, **joint)
                torch.cuda.synchronize()
                ids, ms = (ctypes.c_int * 64)(), (ctypes.c_float * 64)()
                merges = lib.cfx_profile_read(ctx, ids, ms, 64)
                lib.cfx_profile_enable(ctx, 0, 0, 1)
                n1 = ctypes.c_ulonglong(0)
                assert lib.cfx_attn_fwd_launches(ctx, ctypes.byref(n1)) == 0
                n_waits, n_sdpa, steady = len(waits), len(sdpas), len(ran) == 1
                assert out.dtype == dtype and tuple(out.shape) == shape and out.is_contiguous()
                assert lse.dtype == torch.float32 and tuple(lse.shape) == (shape[0], shape[2], shape[1])
                cache = cm.compact_cache()
                states = {(r, nm): bits(cache.get_base(f"{l}-{r}-{nm}")).copy() for r in range(WL) for nm in ("k", "v")}
                # the float64 witness over the K,V the rank holds: its own, then the peers' reconstructed states in ring order
                kk = [k] + [cache.get_base(f"{l}-{(0 - t) % WL}-k").view(shape) for t in range(1, WL)]
                vv = [v] + [cache.get_base(f"{l}-{(0 - t) % WL}-v").view(shape) for t in range(1, WL)]
                if joint:
                    kk[0], vv[0] = torch.cat([jk, k], dim=1), torch.cat([jv, v], dim=1)
                    kk = [torch.cat(kk, dim=1)]
                    vv = [torch.cat(vv, dim=1)]
                ref = W.reference_and_bound(q.float().cpu().numpy(), [t.float().cpu().numpy() for t in kk], [t.float().cpu().numpy() for t in vv],
                                            shape[-1] ** -0.5, dname)
                if mode == "native" and steady:                  # the one launch: held to ITS bound; the sdpa path to the tolerance its own test uses
                    W.check(out.float().cpu().numpy(), lse.transpose(1, 2).cpu().numpy(), ref, f"compact_fwd native {s, l}")
                else:
                    torch.testing.assert_close(out.float().cpu(), torch.from_numpy(ref[0]).float(), rtol=2e-3, atol=2e-3 if dtype == torch.float16 else 1.6e-2)
                    torch.testing.assert_close(lse.transpose(1, 2).cpu(), torch.from_numpy(ref[1]).float(), rtol=2e-3, atol=2e-3)
                rows[s, l] = dict(out=out.clone(), lse=lse.clone(), lse_stride=lse.stride(), states=states, steady=steady, joint=bool(joint),
                                  attn=n1.value - n0.value, sdpa=n_sdpa, merges=merges, waits=n_waits)
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


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("lane", ["off", "auto"])
def test_compact_fwd_native_attention(monkeypatch, lane, dtype):
    """the same seeded sequence with attention="sdpa" and "native": the K,V states of every rank bit-identical between the two runs; out
    and lse of a native steady layer within the derived bound of the float64 witness over the states the rank holds (inside _run_steps),
    in the sdpa path's types, shapes and strides; per steady layer exactly ONE attention launch, no SDPA call, no merge launch and - on
    the lane - W-1 stand-alone flag waits more than the sdpa path's call makes; the binding calls and a call with joint tensors take today's path."""
    sdpa = _run_steps(monkeypatch, lane, dtype, "sdpa")
    native = _run_steps(monkeypatch, lane, dtype, "native")
    assert sdpa.keys() == native.keys()
    steady = []
    for key in sorted(sdpa):
        a, b = sdpa[key], native[key]
        for sk in a["states"]:
            assert np.array_equal(a["states"][sk], b["states"][sk]), (key, sk)
        assert a["steady"] == b["steady"] and a["lse_stride"] == b["lse_stride"] and a["out"].stride() == b["out"].stride()
        assert a["attn"] == 0, f"{key}: the sdpa mode made an attention launch"
        if a["steady"]:
            steady.append(key)
            # (the lean loop asks the fused op once per layer whether it takes the shape: one trial call at a layer's first steady run)
            assert a["sdpa"] in (WL, WL + 1) and a["merges"] == WL, f"{key}: the sdpa path made {a['sdpa']} SDPA calls, {a['merges']} merges"
            assert b["attn"] == 1 and b["sdpa"] == 0 and b["merges"] == 0, f"{key}: native made {b['attn']} launches, {b['sdpa']} SDPA calls, {b['merges']} merges"
            # (the sdpa path's waits ride inside its merge launches: what its call makes besides - the hand-over to and from the lane's
            # compute stream - native makes too, plus one stand-alone wait per peer flag)
            assert b["waits"] - a["waits"] == (WL - 1 if lane == "auto" else 0), f"{key}: {a['waits']} / {b['waits']} flag waits (sdpa / native)"
        else:                                                   # the binding calls, and the calls with joint tensors: today's path, call for call
            assert b["attn"] == 0 and b["sdpa"] == a["sdpa"] > 0 and b["merges"] == a["merges"], (key, a["sdpa"], b["sdpa"], a["merges"], b["merges"])
            rt = 2.0 ** (-7 if dtype == torch.bfloat16 else -10)
            torch.testing.assert_close(b["out"].float(), a["out"].float(), rtol=rt, atol=rt)
        assert not (a["joint"] and a["steady"]), f"{key}: a call with joint tensors ran the steady layer"
    print(f"lane {lane}: steady (step, layer) {steady}")
    assert {(3, 0), (3, 1), (4, 0), (4, 1)} <= set(steady), steady
    assert any(v["joint"] for v in sdpa.values())
