"""cfx_attn_merge_many on the GPU (-m gpu): all of a layer's attention blocks merged in ONE launch, against the float64 witness and the
derived bound of tests/_merge_many_f64.py over every head dim, row shape, block count, element type, layout, output form, gap class,
offset and magnitude the entry point accepts; the 16-bit output form against the fp32 one; a single block; the chain; the launch count;
hipGraph replay; and compact_fwd with configure(attn_merge="once").  Every test fails on a library without the entry point."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import _merge_f64 as M
import _merge_many_f64 as N
import bf16_contract as BC

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BSHD, FIRST, OUT_F32, BF = 1, 2, 4, 0x100
KID_ATTN_MERGE = 30
NS = (1, 2, 3, 8, 16)
bits = BC.torch_bits


@pytest.fixture(autouse=True)
def _collector(tmp_path):
    from compactfusion_amd.collector import collector
    collector.init(collector.Collector(str(tmp_path), enabled=False))
    yield


def _lib_ctx():
    from compactfusion_amd import _lib, codecs as K
    return _lib.load(), K.context(0)


def _cases():
    out, i, classes = [], 0, list(M.GAPS)

    def add(dtype, shape, n, gap, offset, mag):
        B, S, H, D = shape
        out.append(dict(dtype=dtype, shape=shape, n=n, gap=gap, offset=offset, mag=mag,
                        id=f"{dtype}-{B}x{S}x{H}x{D}-n{n}-{gap}-off{int(offset)}-{mag}"))
    for D in M.HEAD_DIMS:                        # 1 .. 64 lanes a row; 42 rows: no multiple of the workgroup for any group width; 256 rows
        for shape in ((2, 7, 3), (2, 16, 8)):
            add(("fp16", "bf16")[i % 2], shape + (D,), NS[i % 5], classes[(i // 2) % 5], (0.0, 300.0, -300.0)[i % 3], "unit")
            i += 1
    for dtype in ("fp16", "bf16"):
        for gap in classes:                      # every gap class at offsets 0 and +-300, and with values at the top of the type's range
            for offset in (0.0, 300.0, -300.0):
                add(dtype, (2, 5, 2, 40), NS[1:][i % 4], gap, offset, "unit")
                i += 1
            add(dtype, (1, 6, 3, 72), (3, 8, 16)[i % 3], gap, 0.0, "max")
        for shape in ((3, 1, 5), (2, 9, 1), (1, 5, 3)):          # S = 1, H = 1, B = 1
            add(dtype, shape + ((24, 136)[i % 2],), NS[i % 5], classes[i % 5], (300.0, -300.0, 0.0)[i % 3], "unit")
            i += 1
    return out


CASES = _cases()
FLUX_CASE = dict(dtype="bf16", shape=(1, 544, 24, 128), n=8, gap="unit", offset=0.0, mag="unit", id="bf16-1x544x24x128-n8-unit-off0-unit")


def test_case_list_covers_what_it_claims():
    assert {c["shape"][3] for c in CASES} >= set(M.HEAD_DIMS) and {c["n"] for c in CASES} == set(NS)
    for D in M.HEAD_DIMS:
        assert {c["shape"][:3] for c in CASES if c["shape"][3] == D} >= {(2, 7, 3), (2, 16, 8)}
    for dtype in ("fp16", "bf16"):
        mine = [c for c in CASES if c["dtype"] == dtype]
        assert {(c["gap"], c["offset"]) for c in mine} >= {(g, o) for g in M.GAPS for o in (0.0, 300.0, -300.0)}
        assert {c["gap"] for c in mine if c["mag"] == "max"} == set(M.GAPS)
        assert {c["n"] for c in mine} == set(NS)
        assert any(c["shape"][1] == 1 for c in mine) and any(c["shape"][2] == 1 for c in mine) and any(c["shape"][0] == 1 for c in mine)


def _device_blocks(case, blocks, bshd):
    """the case's blocks on the device: out in the element type - (B,S,H,D) contiguous, or (B,H,S,D) underneath -, lse fp32 (B,H,S)"""
    tdt = torch.float16 if case["dtype"] == "fp16" else torch.bfloat16
    outs, lses = [], []
    for ob, lb in blocks:
        o = torch.from_numpy(ob).to(tdt).cuda()
        assert torch.equal(o.float().cpu(), torch.from_numpy(ob))
        outs.append(o.contiguous() if bshd else o.transpose(1, 2).contiguous())
        lses.append(torch.from_numpy(lb).permute(0, 2, 1).contiguous().cuda())
    return tdt, outs, lses


def _many(lib, ctx, case, outs, lses, bshd, f32, out=None, lse=None, stream=None):
    B, S, H, D = case["shape"]
    tdt = outs[0].dtype
    n = len(outs)
    if out is None:
        out = torch.full((B, S, H, D), float("nan"), dtype=torch.float32 if f32 else tdt, device="cuda")
        lse = torch.full((B, S, H), float("nan"), dtype=torch.float32, device="cuda")
    P = ctypes.c_void_p * n
    flags = (BSHD if bshd else 0) | (BF if tdt == torch.bfloat16 else 0) | (OUT_F32 if f32 else 0)
    sh = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    rc = lib.cfx_attn_merge_many(ctx, n, P(*[t.data_ptr() for t in outs]), P(*[t.data_ptr() for t in lses]), B, S, H, D, flags,
                                 out.data_ptr(), lse.data_ptr(), sh)
    assert rc == 0, lib.cfx_last_error_string(ctx)
    return out, lse


def _chain(lib, ctx, case, outs, lses, bshd):
    B, S, H, D = case["shape"]
    out = torch.full((B, S, H, D), float("nan"), dtype=torch.float32, device="cuda")
    lse = torch.full((B, S, H), float("nan"), dtype=torch.float32, device="cuda")
    sh = torch.cuda.current_stream().cuda_stream
    for i, (bo, bl) in enumerate(zip(outs, lses)):
        flags = (BSHD if bshd else 0) | (BF if bo.dtype == torch.bfloat16 else 0) | (FIRST if i == 0 else 0)
        rc = lib.cfx_attn_merge_ex(ctx, out.data_ptr(), lse.data_ptr(), bo.data_ptr(), bl.data_ptr(), B, S, H, D, flags, None, 0, None, sh)
        assert rc == 0, lib.cfx_last_error_string(ctx)
    return out, lse


def _launches(lib, ctx, fn):
    """what fn() returns, and how many KID_ATTN_MERGE launches it made"""
    assert lib.cfx_profile_enable(ctx, 64, 1 << KID_ATTN_MERGE, 1) == 0
    try:
        res = fn()
        torch.cuda.synchronize()
        ids, ms = (ctypes.c_int * 64)(), (ctypes.c_float * 64)()
        n = lib.cfx_profile_read(ctx, ids, ms, 64)
        assert all(ids[i] == KID_ATTN_MERGE for i in range(n))
    finally:
        lib.cfx_profile_enable(ctx, 0, 0, 1)
    return res, n


def _same_bits(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    v = torch.int16 if a.element_size() == 2 else torch.int32
    return torch.equal(a.contiguous().view(v), b.contiguous().view(v))


def _check_case(case, with_chain=True):
    lib, ctx = _lib_ctx()
    blocks = M.build(case)
    n = case["n"]
    for bshd in (1, 0):
        tdt, outs, lses = _device_blocks(case, blocks, bshd)
        (o32, l32), launched = _launches(lib, ctx, lambda: _many(lib, ctx, case, outs, lses, bshd, True))
        assert launched == 1, f"{launched} merge launches"
        o16, l16 = _many(lib, ctx, case, outs, lses, bshd, False)
        torch.cuda.synchronize()
        fo, fl = N.check(o32.cpu().numpy(), l32.cpu().numpy(), blocks, f"cfx_attn_merge_many, {'BSHD' if bshd else 'BHSD'}")
        print(f"{case['id']} {'BSHD' if bshd else 'BHSD'}: {fo:.3f} / {fl:.3f} of the bound (out / lse)")
        # the element-type output is the nearest-even rounding of the fp32 output of the same arithmetic, lse the same bits
        assert o16.dtype == tdt and _same_bits(o16, o32.to(tdt)) and _same_bits(l16, l32)
        if n == 1:
            assert _same_bits(o16, outs[0] if bshd else outs[0].transpose(1, 2)) and _same_bits(l32, lses[0].permute(0, 2, 1))
            assert torch.equal(o32, (outs[0] if bshd else outs[0].transpose(1, 2)).float())
        if with_chain:
            (co, cl), launched = _launches(lib, ctx, lambda: _chain(lib, ctx, case, outs, lses, bshd))
            assert launched == n, f"the chain made {launched} launches for {n} blocks"
            M.check(co.cpu().numpy(), cl.cpu().numpy(), blocks, "cfx_attn_merge_ex chain")
    assert lib.cfx_gate_errors(ctx) == 0


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_kernel_against_witness_and_bound(case):
    """both layouts and both output forms of every case: the fp32 result within the derived bound of the float64 witness; the 16-bit
    result its nearest-even rounding; n = 1 the block's own bits; ONE launch where the chain - held to ITS bound of the same float64
    function - makes n."""
    _check_case(case)


def test_flux_shape():
    """(1, 544, 24, 128), 8 blocks, bf16: the shard compact_fwd merges on FLUX"""
    _check_case(FLUX_CASE)


def test_python_entry_takes_the_native_launch():
    """merge_blocks on SDPA-shaped GPU tensors is the one launch (both layouts, both output types); more than 16 blocks are refused"""
    from compactfusion_amd.compact import attention as A
    lib, ctx = _lib_ctx()
    case = dict(dtype="bf16", shape=(2, 7, 3, 72), n=8, gap="unit", offset=0.0, mag="unit", id="python-entry")
    blocks = M.build(case)
    for bshd in (1, 0):
        tdt, outs, lses = _device_blocks(case, blocks, bshd)
        outs = outs if bshd else [o.transpose(1, 2) for o in outs]                  # (B,S,H,D) views, as block_attention returns them
        for od in (None, tdt):
            (out, lse), launched = _launches(lib, ctx, lambda: A.merge_blocks(outs, lses, od))
            assert launched == 1 and out.dtype == (od or torch.float32) and out.is_contiguous() and tuple(lse.shape) == (2, 7, 3, 1)
            if od is None:
                N.check(out.cpu().numpy(), lse.squeeze(-1).cpu().numpy(), blocks, "merge_blocks")
                o32 = out
            else:
                assert _same_bits(out, o32.to(tdt))
    with pytest.raises(ValueError, match="at most 16"):
        A.merge_blocks(outs * 3, lses * 3)


def test_hipgraph_replay():
    """the launch captured at n = 8 and replayed 3 times, the inputs rewritten between replays: every replay within the bound"""
    lib, ctx = _lib_ctx()
    case = dict(dtype="fp16", shape=(2, 7, 3, 136), n=8, gap="unit", offset=0.0, mag="unit", id="graph-0")
    tdt, outs, lses = _device_blocks(case, M.build(case), 1)
    out = torch.full(case["shape"], float("nan"), dtype=torch.float32, device="cuda")
    lse = torch.full(case["shape"][:3], float("nan"), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            _many(lib, ctx, case, outs, lses, 1, True, out, lse, side.cuda_stream)
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "capture must not execute"
    for rep, (gap, offset) in enumerate((("mid", 300.0), ("zero", -300.0), ("unit", 0.0))):
        c = dict(case, gap=gap, offset=offset, id=f"graph-{rep + 1}")
        blocks = M.build(c)
        _, o2, l2 = _device_blocks(c, blocks, 1)
        for dst, src in zip(outs + lses, o2 + l2):
            dst.copy_(src)
        out.fill_(float("nan"))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        fo, fl = N.check(out.cpu().numpy(), lse.cpu().numpy(), blocks, f"replay {rep}")
        print(f"replay {rep}: {fo:.3f} / {fl:.3f} of the bound")
    assert lib.cfx_gate_errors(ctx) == 0


# ---- compact_fwd with configure(attn_merge="once") -------------------------------------------------------------------------------------
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
    """L layers x STEPS steps of compact_fwd, 4 logical ranks looped back, 1-bit codec, configure(attn_merge=mode).  Per (step, layer):
    out, lse, the K,V states of every rank, whether the steady layer ran, the id-30 launches and the cfx_flag_wait calls."""
    from compactfusion_amd import _lib, codecs as K, config, exchange
    from compactfusion_amd.collector import collector
    from compactfusion_amd.compact import ring, main as cm, xlayer
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig
    from compactfusion_amd.compact.attention import block_attention, update_out_and_lse
    from compactfusion_amd.prof import Profiler
    lib = _lib.load()
    ctx = K.context(0)
    config.reset()
    monkeypatch.setenv("CFX_ATTN_MERGE", mode)
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
    ran, waits = [], []
    orig_run, orig_wait = ring._SteadyLayer.run, lib.cfx_flag_wait
    monkeypatch.setattr(ring._SteadyLayer, "run", lambda self, *a: (ran.append(self), orig_run(self, *a))[1])
    monkeypatch.setattr(lib, "cfx_flag_wait", lambda *a: (waits.append(a), orig_wait(*a))[1])
    rows = {}
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
            for l in range(L):
                q, k, v = qs[l][s].cuda(), ks[l][s].cuda(), vs[l][s].cuda()
                torch.cuda.synchronize()
                del ran[:], waits[:]
                assert lib.cfx_profile_enable(ctx, 64, 1 << KID_ATTN_MERGE, 1) == 0
                out, lse, _ = ring.compact_fwd(q, k, v, causal=False, mod_idx=l, current_iter=s)
                torch.cuda.synchronize()
                ids, ms = (ctypes.c_int * 64)(), (ctypes.c_float * 64)()
                n = lib.cfx_profile_read(ctx, ids, ms, 64)
                lib.cfx_profile_enable(ctx, 0, 0, 1)
                n_waits, steady = len(waits), len(ran) == 1
                assert out.dtype == dtype and tuple(out.shape) == shape and out.is_contiguous()
                assert lse.dtype == torch.float32 and tuple(lse.shape) == (shape[0], shape[2], shape[1])
                cache = cm.compact_cache()
                states = {(r, nm): bits(cache.get_base(f"{l}-{r}-{nm}")).copy() for r in range(WL) for nm in ("k", "v")}
                ro = rl = None                   # the eager ring formula on the K,V the rank holds (tests/test_gpu_bf16.py)
                for t in range(WL):
                    kk = k if t == 0 else cache.get_base(f"{l}-{(0 - t) % WL}-k").view(shape)
                    vv = v if t == 0 else cache.get_base(f"{l}-{(0 - t) % WL}-v").view(shape)
                    bo, bl = block_attention(q, kk, vv, 0.0, shape[-1] ** -0.5, causal=False)
                    ro, rl = update_out_and_lse(ro, rl, bo, bl)
                torch.testing.assert_close(out.float(), ro.to(dtype).float(), rtol=2e-3, atol=2e-3)
                torch.testing.assert_close(lse, rl.squeeze(-1).transpose(1, 2), rtol=2e-3, atol=2e-3)
                rows[s, l] = dict(out=out.clone(), lse=lse.clone(), lse_stride=lse.stride(), states=states, steady=steady,
                                  fast=bool(ran and ran[0]._fast), launches=n, waits=n_waits)
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
def test_compact_fwd_merging_once(monkeypatch, lane, dtype):
    """the same seeded sequence with attn_merge="chain" and "once": out and lse within rtol = atol = 2e-3 of the eager ring formula on the
    K,V the rank holds (inside _run_steps), in the chain's types, shapes and views; the K,V states of every rank bit-identical between
    the two runs; and on a steady layer ONE merge launch where the chain makes W, with - on the lane - W-1 more cfx_flag_wait launches
    than the chain's call makes."""
    chain = _run_steps(monkeypatch, lane, dtype, "chain")
    once = _run_steps(monkeypatch, lane, dtype, "once")
    assert chain.keys() == once.keys()
    steady = []
    for key in sorted(chain):
        a, b = chain[key], once[key]
        for sk in a["states"]:
            assert np.array_equal(a["states"][sk], b["states"][sk]), (key, sk)
        assert a["steady"] == b["steady"] and a["lse_stride"] == b["lse_stride"]
        # (the two fp32 results agree to a few fp32 ulps: their roundings to the element type are equal or adjacent)
        torch.testing.assert_close(b["out"].float(), a["out"].float(), rtol=2.0 ** (-7 if dtype == torch.bfloat16 else -10), atol=1e-6)
        torch.testing.assert_close(b["lse"], a["lse"], rtol=2e-5, atol=2e-5)
        if a["steady"]:
            steady.append(key)
            assert a["fast"] and b["fast"], f"{key}: the steady layer left the lean loop"
            assert a["launches"] == WL and b["launches"] == 1, f"{key}: {a['launches']} / {b['launches']} merge launches (chain / once)"
            assert b["waits"] - a["waits"] == (WL - 1 if lane == "auto" else 0), f"{key}: {a['waits']} / {b['waits']} flag waits (chain / once)"
        else:
            assert b["launches"] == a["launches"], f"{key}: the binding call keeps the chain"
    print(f"lane {lane}: steady (step, layer) {steady}")
    assert {(3, 0), (3, 1), (4, 0), (4, 1)} <= set(steady), steady
