"""cfx_attn_fwd_blocks_hd on the GPU (-m gpu): the one-launch attention at the head dims between 64 and 128 (72, 80, .. 120) against the
float64 witness and the derived bound of tests/_attn_var_f64.py on every case of tests/_attn_hd_cases.py, fp16 and bf16; bit for bit
against cfx_attn_fwd_blocks_var on the same tensors zero-padded to D = 128 (what pins the walk to the existing contract); q and every
block carved out of a NaN-filled allocation (an over-read of a row shows as NaN); every query tile; hipGraph replay; every C-ABI refusal;
attention_blocks and compact_fwd at D = 72; patch_gather_fwd as ONE launch without torch.cat, two rank processes on one GPU.  Every test
fails on a library without the entry point or a package that keeps the 64 / 128 limit."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch

import _attn_hd_cases as HC
import _attn_var_cases as VC
import _attn_var_f64 as VW
import bf16_contract as BC

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _harness():
    """tests/test_gpu_attn_var.py's loop-back harness for compact_fwd on the steady layer (`_run_steps`) and its small helpers, as a module
    object of this file's own: its shapes are set to D = 72 below, and the test module pytest collects keeps its own"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_attn_var_harness", os.path.join(HERE, "test_gpu_attn_var.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TV = _harness()
BF = 0x100
TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
bits = BC.torch_bits
_lib_ctx, _dev, _count, _outs, _same_bits = TV._lib_ctx, TV._dev, TV._count, TV._outs, TV._same_bits
_refs = {}


def ref_of(case, dtype):
    """the case's inputs and its witness / bound, computed once and left unchanged"""
    key = (case["id"], dtype)
    if key not in _refs:
        q, ks, vs, scale = VC.build(case, dtype)
        _refs[key] = (q, ks, vs, scale, VW.reference_and_bound(q, ks, vs, scale, dtype))
    return _refs[key]


def _hd(lib, ctx, q, ks, vs, scale, out=None, lse=None, stream=None, fn=None):
    """cfx_attn_fwd_blocks_hd (or `fn`: cfx_attn_fwd_blocks_var, the same arguments); every block (B, Sk_i, H, D) contiguous"""
    B, Sq, H, D = q.shape
    n = len(ks)
    assert q.is_contiguous() and all(k.is_contiguous() and v.is_contiguous() and k.shape == v.shape and (k.shape[0], k.shape[2], k.shape[3]) == (B, H, D)
                                     for k, v in zip(ks, vs))
    if out is None:
        out, lse = _outs(q)
    P = ctypes.c_void_p * n
    sh = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    rc = (fn or lib.cfx_attn_fwd_blocks_hd)(ctx, n, q.data_ptr(), P(*[t.data_ptr() for t in ks]), P(*[t.data_ptr() for t in vs]),
                                            (ctypes.c_int * n)(*[t.shape[1] for t in ks]), B, Sq, H, D, scale, BF if q.dtype == torch.bfloat16 else 0,
                                            out.data_ptr(), lse.data_ptr(), sh)
    assert rc == 0, lib.cfx_last_error_string(ctx)
    return out, lse


@pytest.mark.parametrize("dtype", list(TDT))
def test_kernel_against_witness_and_bound(dtype):
    """out and lse of EVERY case of tests/_attn_hd_cases.py within the derived bound of the float64 witness - the bound of the TRUE D -,
    each in ONE counted launch; a single key returns v's bits"""
    lib, ctx = _lib_ctx()
    for case in HC.CASES:
        q, ks, vs, scale, ref = ref_of(case, dtype)
        dq, dks, dvs = _dev(q, dtype), [_dev(k, dtype) for k in ks], [_dev(v, dtype) for v in vs]
        n0 = _count(lib, ctx)
        out, lse = _hd(lib, ctx, dq, dks, dvs, scale)
        torch.cuda.synchronize()
        assert _count(lib, ctx) == n0 + 1, case["id"]
        fo, fl = VW.check(out.float().cpu().numpy(), lse.cpu().numpy(), ref, f"cfx_attn_fwd_blocks_hd, {case['id']} {dtype}")
        print(f"{case['id']} {dtype}: {fo:.3f} / {fl:.3f} of the bound (out / lse)")
        if case["sks"] == [1]:
            assert _same_bits(out, dvs[0].expand_as(out)), case["id"]
    assert lib.cfx_gate_errors(ctx) == 0


@pytest.mark.parametrize("dtype", list(TDT))
@pytest.mark.parametrize("D", HC.DIMS)
def test_zero_padded_to_128_is_the_var_launch_bit_for_bit(D, dtype):
    """q, K and V zero-padded to D = 128 through cfx_attn_fwd_blocks_var with the same softmax_scale and the same sks: its out[..., :D]
    and its lse ARE the new launch's, bit for bit - B = 2, H = 3, lists with tails, values to +-1e4 (ramp) among them"""
    lib, ctx = _lib_ctx()
    for kind, sks, Sq in (("gauss", [100, 37, 128, 5], 129), ("gauss", [65, 64, 63], 33), ("ramp", [65, 64, 63], 80), ("gauss", list(range(1, 17)), 1)):
        case = dict(B=2, Sq=Sq, sks=sks, H=3, D=D, kind=kind, id=f"pad-{kind}-q{Sq}-{VC._tag(sks)}-d{D}")
        q, ks, vs, scale = VC.build(case, dtype)
        dq, dks, dvs = _dev(q, dtype), [_dev(k, dtype) for k in ks], [_dev(v, dtype) for v in vs]
        pad = lambda t: torch.nn.functional.pad(t, (0, 128 - D)).contiguous()           # noqa: E731
        pq, pks, pvs = pad(dq), [pad(k) for k in dks], [pad(v) for v in dvs]
        assert pq.shape[-1] == 128 and not pq[..., D:].any()
        o1, l1 = _hd(lib, ctx, dq, dks, dvs, scale)
        o0, l0 = _hd(lib, ctx, pq, pks, pvs, scale, fn=lib.cfx_attn_fwd_blocks_var)
        torch.cuda.synchronize()
        assert _same_bits(o1, o0[..., :D].contiguous()) and _same_bits(l1, l0), case["id"]
        assert not o0[..., D:].any()                                                     # (the padded columns of V: zeros out)
        VW.check(o1.float().cpu().numpy(), l1.cpu().numpy(), VW.reference_and_bound(q, ks, vs, scale, dtype), case["id"])


@pytest.mark.parametrize("dtype", list(TDT))
def test_rows_carved_out_of_a_nan_filled_allocation(dtype):
    """q and every K, V block carved out of ONE allocation filled with NaN, 256 bytes or more of NaN after each; H = 1, so the row after a
    tensor's last is NaN: a fragment, a staged chunk or an LDS column read past D - past the last row - would make out or lse NaN
    instead of passing unseen (it stays inside the allocation: nothing faults).  Finite and within the bound, every D"""
    lib, ctx = _lib_ctx()
    for D in HC.DIMS:
        case = dict(B=1, Sq=33, sks=[65, 64, 63], H=1, D=D, kind="gauss", id=f"nan-d{D}")
        q, ks, vs, scale = VC.build(case, dtype)
        hosts = [q] + ks + vs
        gap = 256 // 2 + 8
        pool = torch.full((sum(t.size + gap for t in hosts) + gap,), float("nan"), dtype=TDT[dtype], device="cuda")
        assert pool.data_ptr() % 16 == 0
        views, at = [], gap
        for t in hosts:
            at = (at + 7) // 8 * 8                                                   # 16-byte aligned
            v = pool[at:at + t.size].view(t.shape)
            v.copy_(_dev(t, dtype))
            views.append(v)
            at += t.size + gap
        dq, dks, dvs = views[0], views[1:1 + len(ks)], views[1 + len(ks):]
        assert torch.isnan(pool[dq.numel() + gap:dq.numel() + 2 * gap - 8]).all()       # the 256 bytes behind q's last row
        out, lse = _hd(lib, ctx, dq, dks, dvs, scale)
        torch.cuda.synchronize()
        assert torch.isfinite(out).all() and torch.isfinite(lse).all(), f"D = {D}: NaN read from past a row"
        VW.check(out.float().cpu().numpy(), lse.cpu().numpy(), VW.reference_and_bound(q, ks, vs, scale, dtype), case["id"])


@pytest.mark.parametrize("dtype", list(TDT))
def test_every_query_tile_returns_the_same_bits(dtype):
    """cfx_set_attn_qtile: 64, 128 and 256 query rows a workgroup (the staging loop's guarded pass differs with the thread count) give
    the library's choice's bits; Sq = 129: 5 waves"""
    lib, ctx = _lib_ctx()
    for D in (72, 88, 104, 120):
        case = dict(B=2, Sq=129, sks=[100, 37, 128, 5], H=3, D=D, kind="gauss", id=f"qtile-d{D}")
        q, ks, vs, scale = VC.build(case, dtype)
        dq, dks, dvs = _dev(q, dtype), [_dev(k, dtype) for k in ks], [_dev(v, dtype) for v in vs]
        out, lse = _hd(lib, ctx, dq, dks, dvs, scale)
        try:
            for rows in (64, 128, 256):
                assert lib.cfx_set_attn_qtile(ctx, rows) == 0
                o, l = _hd(lib, ctx, dq, dks, dvs, scale)
                torch.cuda.synchronize()
                assert _same_bits(o, out) and _same_bits(l, lse), (D, rows)
        finally:
            assert lib.cfx_set_attn_qtile(ctx, 0) == 0
        VW.check(out.float().cpu().numpy(), lse.cpu().numpy(), VW.reference_and_bound(q, ks, vs, scale, dtype), "the library's tile")


def test_hipgraph_replay():
    """ONE launch at D = 72 captured and replayed 3 times, the inputs rewritten in place between replays: every replay within the bound"""
    lib, ctx = _lib_ctx()
    base = dict(B=2, Sq=80, sks=[100, 37, 128, 5], H=3, D=72)
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
            _hd(lib, ctx, dq, dks, dvs, scale, out, lse, side.cuda_stream)
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "capture must not execute"
    assert _count(lib, ctx) == n0 + 1
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
    """every refusal on live device pointers, in cfx_attn_fwd_blocks_var's order - NULL, flag, shape / n / key counts / head dim / scale,
    alignment -; each returns before any launch: the count does not move and the outputs keep their NaNs"""
    lib, ctx = _lib_ctx()
    NULL, SHAPE, ALIGN, CODEC = -1, -2, -3, -4
    B, Sq, H, D = 1, 4, 2, 72
    q = torch.zeros(B, Sq, H, D, dtype=torch.float16, device="cuda")
    kv = [torch.zeros(B, 4 + i, H, D + 8, dtype=torch.float16, device="cuda") for i in range(17)]      # (spare elements: room for a misaligned pointer)
    out = torch.full((B, Sq, H, 128 + 8), float("nan"), dtype=torch.float16, device="cuda")
    lse = torch.full((B, Sq, H + 4), float("nan"), dtype=torch.float32, device="cuda")
    P, I = ctypes.c_void_p * 17, ctypes.c_int * 17
    ks = P(*[t.data_ptr() for t in kv])
    sk = I(*[4 + i for i in range(17)])
    f = lib.cfx_attn_fwd_blocks_hd
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
        (CODEC, (ctx, 0, qp, ks, ks, nokeys, B, Sq, H, 64, 0.0, 0x40, op + 2, lp, sh)),        # the flag before n, the shape, the scale and the alignment
        (CODEC, (ctx, 2, qp, ks, ks, sk, B, Sq, H, D, 0.125, 1, op, lp, sh)),
        (SHAPE, (ctx, 17, qp, ks, ks, sk, B, Sq, H, D, 0.125, 0, op + 2, lp, sh)),             # n, sizes, key counts, head dim, scale before the alignment
        (SHAPE, (ctx, 0, qp, ks, ks, sk, B, Sq, H, D, 0.125, BF, op + 2, lp, sh)),
        (SHAPE, (ctx, 2, qp, ks, ks, nokeys, B, Sq, H, D, 0.125, 0, op + 2, lp, sh)),
        (SHAPE, (ctx, 2, qp, ks, ks, sk, B, 0, H, D, 0.125, 0, op + 2, lp, sh)),
        (SHAPE, (ctx, 2, qp, ks, ks, sk, B, Sq, H, 64, 0.125, 0, op, lp, sh)),                 # 64 and 128 are the other entry points'
        (SHAPE, (ctx, 2, qp, ks, ks, sk, B, Sq, H, 128, 0.125, BF, op, lp, sh)),
        (SHAPE, (ctx, 2, qp, ks, ks, sk, B, Sq, H, 76, 0.125, 0, op, lp, sh)),
        (SHAPE, (ctx, 2, qp, ks, ks, sk, B, Sq, H, 136, 0.125, 0, op, lp, sh)),
        (SHAPE, (ctx, 2, qp, ks, ks, sk, B, Sq, H, D, float("nan"), 0, op + 2, lp, sh)),
        (SHAPE, (ctx, 2, qp, ks, ks, sk, B, Sq, H, D, -1.0, 0, op + 2, lp, sh)),
        (ALIGN, (ctx, 2, qp, ks, ks, sk, B, Sq, H, D, 0.125, 0, op + 2, lp, sh)),
        (ALIGN, (ctx, 2, qp, ks, ks, sk, B, Sq, H, D, 0.125, 0, op, lp + 4, sh)),
        (ALIGN, (ctx, 2, qp, bad_al, ks, sk, B, Sq, H, D, 0.125, 0, op, lp, sh)),
        (ALIGN, (ctx, 2, qp, ks, bad_al, sk, B, Sq, H, D, 0.125, BF, op, lp, sh)),
    ]
    for want, a in steps:
        assert f(*a) == want, (want, a[1], a[9:12], lib.cfx_last_error_string(ctx))
    torch.cuda.synchronize()
    assert _count(lib, ctx) == n0 and torch.isnan(out).all() and torch.isnan(lse).all()


def test_python_entry_takes_the_launch_at_d72():
    """attention_blocks on GPU tensors of head dim 72 is ONE launch, for equal and for unequal blocks, proved by the counter (before:
    the eager definition); a non-contiguous block still runs the eager definition; more than 16 blocks are refused"""
    from compactfusion_amd.compact import attention as A
    lib, ctx = _lib_ctx()
    for dtype in TDT:
        for sks in ([100, 37, 128, 5], [40, 40, 40]):
            case = dict(B=2, Sq=33, sks=sks, H=3, D=72, kind="gauss", id=f"py-{VC._tag(sks)}")
            q, ks, vs, scale, ref = ref_of(case, dtype)
            dq, dks, dvs = _dev(q, dtype), [_dev(k, dtype) for k in ks], [_dev(v, dtype) for v in vs]
            equal = len(set(sks)) == 1
            assert A.attn_native_var_ok(dq, dks, dvs) and A.attn_native_ok(dq, dks, dvs) == equal
            n0 = A.attn_fwd_launches(0)
            out, lse = A.attention_blocks(dq, dks, dvs)             # the default scale: D ** -0.5
            torch.cuda.synchronize()
            assert A.attn_fwd_launches(0) == n0 + 1, (dtype, sks)
            B, Sq, H, D = q.shape
            assert out.dtype == TDT[dtype] and out.is_contiguous() and tuple(lse.shape) == (B, H, Sq) and lse.stride() == (Sq * H, 1, H)
            VW.check(out.float().cpu().numpy(), lse.transpose(1, 2).cpu().numpy(), ref, "attention_blocks")
            o1, l1 = _hd(lib, ctx, dq, dks, dvs, scale)
            assert _same_bits(out, o1) and _same_bits(lse.transpose(1, 2), l1)
            n1 = A.attn_fwd_launches(0)
            odd = [dks[0].transpose(1, 2).contiguous().transpose(1, 2)] + dks[1:]
            assert not A.attn_native_var_ok(dq, odd, dvs) and not A.attn_native_ok(dq, odd, dvs)
            o2, l2 = A.attention_blocks(dq, odd, dvs, scale)
            assert A.attn_fwd_launches(0) == n1
            VW.check(o2.float().cpu().numpy(), l2.transpose(1, 2).cpu().numpy(), ref, "attention_blocks, eager on the GPU")
            with pytest.raises(ValueError, match="at most 16"):
                A.attention_blocks(dq, dks * 6, dvs * 6, scale)
            assert A.attn_fwd_launches(0) == n1


@pytest.mark.parametrize("dname", list(TDT))
def test_compact_fwd_at_d72_is_one_launch_a_steady_layer(monkeypatch, dname):
    """compact_fwd, W = 4, heads of 72, configure(joint="steady"): attention="native" against attention="sdpa" on the same seeded sequence
    (tests/test_gpu_attn_var.py's loop-back harness at D = 72) - the K,V states of every rank bit-identical call for call; every steady
    call, with joint tensors (W + 1 blocks of unequal length) or without (W equal blocks), exactly ONE attention launch, no SDPA call,
    no merge launch, out / lse within the witness's bound (checked in the harness)"""
    monkeypatch.setattr(TV, "KV", (1, 64, 8, 72))
    monkeypatch.setattr(TV, "QS", (1, 80, 8, 72))
    monkeypatch.setattr(TV, "JS", (1, 16, 8, 72))
    dtype = TDT[dname]
    ref = TV._run_steps(monkeypatch, "off", dtype, "front", "steady", "sdpa")
    got = TV._run_steps(monkeypatch, "off", dtype, "front", "steady", "native")
    assert ref.keys() == got.keys()
    steady = []
    for key in sorted(ref):
        a, b = ref[key], got[key]
        for sk in a["states"]:
            assert np.array_equal(a["states"][sk], b["states"][sk]), (key, sk)
        assert a["steady"] == b["steady"] and a["attn"] == 0
        if b["steady"]:
            steady.append(key)
            assert b["attn"] == 1 and b["sdpa"] == 0 and b["merges"] == 0, f"{key}: native made {b['attn']} launches, {b['sdpa']} SDPA calls, {b['merges']} merges"
    assert {(s, l) for s in (3, 4, 5) for l in range(TV.L)} <= set(steady), steady          # joint (3, 5) and plain (4) calls


# ---- patch_gather_fwd: two rank processes on one GPU -------------------------------------------------------------------------------------
PSTEPS = 4


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _TorchSpy:
    """stands in for compact/patchpara/fwd.py's `torch`: counts torch.cat, passes everything through"""

    def __init__(self):
        self.cats = 0

    def cat(self, *a, **kw):
        self.cats += 1
        return torch.cat(*a, **kw)

    def __getattr__(self, name):
        return getattr(torch, name)


PCONFIGS = [(72, "none"), (72, "front"), (72, "rear"), (64, "none"), (64, "front")]       # D = 64: the SD3 case


def _patch_worker(rank, world, port, out):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    import tempfile
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    import compactfusion_amd
    from compactfusion_amd.collector import collector
    collector.init(collector.Collector(tempfile.mkdtemp(), enabled=False))
    import compactfusion_amd.compact.main as cm
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig, PatchConfig
    from compactfusion_amd.compact import attention as A
    from compactfusion_amd.compact.patchpara import fwd as F
    from compactfusion_amd.compact.ring import compact_fwd
    import _dist_workers as W
    spy = _TorchSpy()
    F.torch = spy
    seen = []

    def record(fn):
        def wrap(q, lk, lv, scale, *a, **kw):
            seen.append(([t.float().cpu().numpy() for t in lk], [t.float().cpu().numpy() for t in lv]))
            return fn(q, lk, lv, scale, *a, **kw)
        return wrap
    F._attn_fwd_native, F._attn_fwd_native_var = record(F._attn_fwd_native), record(F._attn_fwd_native_var)
    res = {}
    for (D, joint), attention in [(c, a) for c in PCONFIGS for a in ("sdpa", "native")]:
        shape, jshape = (1, 64, 16, D), (1, 16, 16, D)
        qs, ks, vs = (W.drift(sd + rank, shape, PSTEPS) for sd in (7, 17, 27))
        jks, jvs = (W.drift(sd, jshape, PSTEPS) for sd in (37, 47))                  # the joint tensors: the same on every rank
        compactfusion_amd.configure(attention=attention)
        for mode, pc in (("sync", PatchConfig(True, False, 1)), ("disp", PatchConfig(True, True, 1, displaced_compact=True))):
            cm.compact_init(CompactConfig(enabled=True, override_with_patch_gather_fwd=True, patch_gather_fwd_config=pc,
                                          compress_func=lambda l, s: T.WARMUP if s == 0 else T.BINARY,
                                          residual=1, ef=True, fastpath=True, comp_rank=-1))
            for step in range(PSTEPS):
                cm.compact_set_step(step)
                kw = dict(joint_tensor_key=jks[step].cuda(), joint_tensor_value=jvs[step].cuda(), joint_strategy=joint) if joint != "none" else {}
                q = qs[step].cuda()
                torch.cuda.synchronize()
                del seen[:]
                spy.cats = 0
                n0 = A.attn_fwd_launches(0)
                out_, lse, _ = compact_fwd(q, ks[step].cuda(), vs[step].cuda(), causal=False, group=None, mod_idx=3, current_iter=step, **kw)
                torch.cuda.synchronize()
                pre = f"d{D}-{joint}/{attention}/{mode}/s{step}/"
                res[pre + "launches"] = np.array([A.attn_fwd_launches(0) - n0])
                res[pre + "cats"] = np.array([spy.cats])
                res[pre + "out"] = out_.float().cpu().numpy()
                res[pre + "lse"] = lse.transpose(1, 2).float().cpu().numpy()              # (B, Sq, H)
                res[pre + "q"] = q.float().cpu().numpy()
                if seen:
                    assert len(seen) == 1
                    res[pre + "nblocks"] = np.array([len(seen[0][0])])
                    for i, (kk, vv) in enumerate(zip(*seen[0])):
                        res[pre + f"k{i}"], res[pre + f"v{i}"] = kk, vv
                for r in range(world):
                    for nm in ("k", "v"):
                        res[pre + f"state_{nm}_{r}"] = bits(cm.compact_cache().get_base(f"3-{nm}-{r}")).copy()
            cm.compact_flush_displaced()
            torch.cuda.synchronize()
            for r in range(world):
                res[f"d{D}-{joint}/{attention}/{mode}/final/state_v_{r}"] = bits(cm.compact_cache().get_base(f"3-v-{r}")).copy()
    compactfusion_amd.configure(attention="sdpa")
    dist.barrier()
    np.savez(out + f".r{rank}.npz", **res)
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def patch_runs(tmp_path_factory):
    """ONE pair of rank processes runs every configuration of PCONFIGS under both settings (a fresh child per rank)"""
    import torch.multiprocessing as mp
    out = str(tmp_path_factory.mktemp("patch_hd") / "patch")
    mp.start_processes(_patch_worker, args=(2, _port(), out), nprocs=2, join=True, start_method="spawn")
    return [dict(np.load(out + f".r{r}.npz")) for r in range(2)]


@pytest.mark.parametrize("D,joint", PCONFIGS)
def test_patch_gather_fwd_is_one_launch_two_processes_one_gpu(patch_runs, D, joint):
    """patch_gather_fwd under configure(attention="native") against the same run under "sdpa": two rank processes (gloo) on one GPU, shards
    (1, 64, 16, D), 1-bit codec, 4 steps, synchronous and displaced compressed gather, without and with joint tensors of 16 keys.  The K,V
    states are bit-identical to the sdpa run's call for call; every call from the second step on is exactly ONE attention launch and no
    torch.cat from fwd.py (the sdpa run: two or more, no launch); out / lse within the bound of the float64 witness over the blocks the
    launch was given - [joint] + states (front), states + [joint] (rear), in rank order.  D = 64 is the SD3 case."""
    nb = 2 + (joint != "none")
    for r in range(2):
        top = f"d{D}-{joint}/"
        g = {k[len(top):]: v for k, v in patch_runs[r].items() if k.startswith(top)}
        for mode in ("sync", "disp"):
            for s in range(PSTEPS):
                a, b = f"sdpa/{mode}/s{s}/", f"native/{mode}/s{s}/"
                for key in [k for k in g if k.startswith(a + "state_")]:
                    assert np.array_equal(g[key], g[b + key[len(a):]]), (r, key)
                assert int(g[a + "launches"][0]) == 0 and int(g[a + "cats"][0]) >= 2, (r, a)
                if s == 0 and b + "nblocks" not in g:
                    continue
                assert int(g[b + "launches"][0]) == 1 and int(g[b + "cats"][0]) == 0, (r, b, g[b + "launches"], g[b + "cats"])
                assert int(g[b + "nblocks"][0]) == nb
                lk, lv = [g[b + f"k{i}"] for i in range(nb)], [g[b + f"v{i}"] for i in range(nb)]
                want = [16, 64, 64] if joint == "front" else ([64, 64, 16] if joint == "rear" else [64, 64])
                assert [k.shape[1] for k in lk] == want
                ref = VW.reference_and_bound(g[b + "q"], lk, lv, D ** -0.5, "fp16")
                fo, fl = VW.check(g[b + "out"], g[b + "lse"], ref, f"patch_gather_fwd native, rank {r} {mode} step {s}")
                print(f"rank {r} {mode} step {s}: {fo:.3f} / {fl:.3f} of the bound")
                np.testing.assert_allclose(g[b + "out"], g[a + "out"], rtol=2e-3, atol=2e-3)      # ... and the sdpa run's result, to SDPA's own tolerance
            for q_ in range(2):
                assert np.array_equal(g[f"sdpa/{mode}/final/state_v_{q_}"], g[f"native/{mode}/final/state_v_{q_}"])
        for s in range(1, PSTEPS):
            assert f"native/sync/s{s}/nblocks" in g and f"native/disp/s{s}/nblocks" in g, (r, s)
