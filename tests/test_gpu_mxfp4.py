"""The MXFP4 wire codec (id 8) on the GPU (-m gpu), in every launch form, over its shape and value domain (tests/_mxfp4_cases.py): packets as
whole byte strings, sender state, receiver reconstruction and peer states against the numpy contract (tests/mxfp4_contract.py) bit for bit
- the non-finite cases as "NaN where the contract has NaN, bits elsewhere" -, no gate error, and every form PROVED by the kernel ids the
call launched (cfx_profile_enable): the stand-alone kernels report top-k's ids 13 / 14, the one-launch layer k_mx_layer id 31.

Forms: cfx_compress_batch / cfx_decompress_batch at batch 1, 2, 16; cfx_compress_batch_gated with loop-back peers (31 alone), the same on a
CU-masked stream below 128 CUs and with cfx_set_gated_launch(0) (13, 14); cfx_set_rows_per_tile (no effect); in place and out of place,
CFX_FLAG_NO_EF, base NULL; plan ops; a captured graph of the layer call and of the p2p layer op; compact_fwd / compact_all_gather_kv with
the lane off and on; two rank processes on one GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _dist_workers as W
import _mxfp4_cases as MC
import _mxfp4_f64_check as F
import mxfp4_contract as M
from _gpu_codec import KID_LAYER, _profile, dev, host, inputs
from oracle import ref_np as R

pytestmark = pytest.mark.gpu

F16 = np.float16
CID = M.CID
KID_C, KID_D = 13, 14            # csrc/cfx_internal.h KID_TOPK_COMPRESS / _DECOMPRESS: what k_mx_compress / k_mx_decompress report
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def oracle(x, base, ef=True):
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        pkt, nb = M.residual_compress(x, base, ef)
    return np.asarray(pkt).view(np.uint16), R.bits(nb)


def same(got, want, what):
    """bits; NaN where the contract has NaN"""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, what
    nan = (want & 0x7FFF) > 0x7C00
    assert ((got[nan] & 0x7FFF) > 0x7C00).all(), f"{what}: not NaN where the contract has NaN"
    bad = got[~nan] != want[~nan]
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} halves differ (first at {int(np.argmax(bad))})"


def same_packet(got, want, what):
    assert np.array_equal(np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)), f"{what}: packet bytes differ"


@pytest.fixture(autouse=True)
def _defaults():
    yield
    from compactfusion_amd import _lib, codecs as K
    K.set_rows_per_tile(0)
    assert _lib.load().cfx_set_gated_launch(K.context(0), 1) == 0


def _plain(x, base, rounds, finite, what):
    """compress + decompress over `rounds` rounds of error feedback; the kernel ids of the first compress and decompress"""
    from compactfusion_amd import _lib, codecs as K
    lib, ctx = _lib.load(), K.context(0)
    N, C = x.shape
    xd = dev(x)
    bd = None if base is None else dev(base)
    state, ids = base, None
    for t in range(rounds):
        pkt_ref, nb_ref = oracle(x, state)
        out = {}

        def comp():
            out["pkt"], out["nb"] = K.compress(CID, xd, bd, N, C, 0, update_cache=True)

        def dec():
            out["rec"] = K.decompress(CID, out["pkt"], bd, N, C, 0)
        if ids is None:
            ids = (_profile(ctx, lib, comp), _profile(ctx, lib, dec))
        else:
            comp()
            dec()
        torch.cuda.synchronize()
        hp, hn = host(out["pkt"]), host(out["nb"]).reshape(N, C)
        same_packet(hp, pkt_ref, f"{what}: packet round {t}")
        same(hn, nb_ref, f"{what}: sender state round {t}")
        same(host(out["rec"]), nb_ref, f"{what}: receiver reconstruction round {t}")
        if finite:
            F.check(x, state, hp, hn)
        bd, state = out["nb"], nb_ref.view(F16).reshape(N, C)
    assert lib.cfx_gate_errors(ctx) == 0
    return ids


def _gated(N, C, ins, rounds, f64=False, NP=3, stream=None):
    """cfx_compress_batch_gated with own error feedback and looped-back peers over rounds, against the contract; the kernel ids of the
    first round.  stream: a raw stream handle (a CU-masked stream), default the current one."""
    from compactfusion_amd import _lib, codecs as K
    lib, ctx = _lib.load(), K.context(0)
    B = len(ins)
    xs = [x for x, _ in ins]
    xd = [dev(x) for x in xs]
    own = [dev(b) for _, b in ins]
    src = [i % B for i in range(NP)]
    peer = [dev(ins[src[g]][1]) for g in range(NP)]
    pk = [torch.zeros(K.packet_halves(CID, N, C, 0), dtype=torch.float16, device="cuda") for _ in range(B)]
    sh = torch.cuda.current_stream().cuda_stream if stream is None else stream
    comp = (_lib.CompItem * B)(*[_lib.CompItem(xd[i].data_ptr(), own[i].data_ptr(), own[i].data_ptr(), pk[i].data_ptr()) for i in range(B)])
    gated = (_lib.DecompItem * NP)(*[_lib.DecompItem(pk[src[g]].data_ptr(), peer[g].data_ptr(), peer[g].data_ptr()) for g in range(NP)])
    torch.cuda.synchronize()

    def go():
        assert lib.cfx_compress_batch_gated(ctx, CID, N, C, 0, _lib.FLAG_UPDATE_CACHE, B, comp, 0, None, NP, gated, None, 0, sh) == 0
    ostate = [np.ascontiguousarray(b).view(np.uint16).copy() for _, b in ins]
    ids = None
    for t in range(rounds):
        if ids is None:
            ids = _profile(ctx, lib, go)
        else:
            go()
        opk, before = [], [s for s in ostate]
        for i in range(B):
            p, nb = oracle(xs[i], ostate[i].view(F16).reshape(N, C))
            opk.append(p)
            ostate[i] = nb.copy()
        torch.cuda.synchronize()
        assert lib.cfx_gate_errors(ctx) == 0
        for i in range(B):
            same_packet(host(pk[i]), opk[i], f"packet round {t} item {i}")
            same(host(own[i]), ostate[i], f"own state round {t} item {i}")
            if f64:
                F.check(xs[i], before[i].view(F16).reshape(N, C), host(pk[i]), host(own[i]).reshape(N, C))
        for g in range(NP):
            same(host(peer[g]), ostate[src[g]], f"peer state round {t} peer {g}")
    torch.cuda.synchronize()
    return ids


# ---- the value domain in the stand-alone and the layer form --------------------------------------------------------------------------
_PARAMS = [(case, N, C) for case in MC.NAMES for N, C in MC.SHAPES]


@pytest.mark.parametrize("case,N,C", _PARAMS, ids=[f"{c}-{n}x{k}" for c, n, k in _PARAMS])
def test_value_domain_stand_alone_and_layer(case, N, C):
    finite = case in MC.FINITE
    reps = MC.reps(case, N, C)
    for rep in range(reps):
        x, base = MC.build(case, N, C, rep=rep)
        ids = _plain(x, base, 2 if rep == 0 else 1, finite, f"{case} rep {rep}")
        assert ids == ([KID_C], [KID_D]), (case, N, C, ids)
    x0, _ = MC.build(case, N, C, nobase=True)
    assert _plain(x0, None, 1, finite, f"{case} base None") == ([KID_C], [KID_D])
    for rep in range(0, reps, 2):
        ins = [MC.build(case, N, C, rep=r % reps) for r in (rep, rep + 1)]
        ids = _gated(N, C, ins, rounds=2 if rep == 0 else 1, f64=finite)
        assert ids == [KID_LAYER], (case, N, C, ids)


def test_layer_of_16_items_at_the_flux_shard():
    """K, V and 14 peers' tensors of (544, 3072) in one k_mx_layer launch: 2 x 204 S workgroups, 14 x 102 D workgroups"""
    N, C = MC.LAYER16
    ins = [MC.build(case, N, C) for case in ("edges", "nonfinite")]
    assert _gated(N, C, ins, rounds=2, NP=14) == [KID_LAYER]


def test_gated_batch_of_16():
    """CFX_MAX_BATCH own tensors and as many looped-back peers in one layer launch"""
    N, C = 5, 320
    ins = [inputs(500 + i, N, C) for i in range(16)]
    assert _gated(N, C, ins, rounds=2, NP=16, f64=True) == [KID_LAYER]


# ---- the fall-back forms of the gated call: below 128 CUs, the one-launch forms switched off; rows per tile has no effect -------------
@pytest.mark.parametrize("N,C", [(5, 320), (17, 576), (64, 3072)])
def test_gated_call_on_a_masked_stream_falls_back(N, C):
    from compactfusion_amd import _lib, codecs as K
    lib, ctx = _lib.load(), K.context(0)
    h = ctypes.c_void_p()
    assert lib.cfx_stream_create_masked(ctx, 0, 64, ctypes.byref(h)) == 0
    try:
        ins = [MC.build("midpoints", N, C), MC.build("random", N, C)]
        assert _gated(N, C, ins, rounds=2, stream=h.value) == [KID_C, KID_D]
    finally:
        torch.cuda.synchronize()
        lib.cfx_stream_destroy(ctx, h)


@pytest.mark.parametrize("N,C", [(5, 320), (17, 576)])
def test_gated_launch_off_and_rows_per_tile(N, C):
    from compactfusion_amd import _lib, codecs as K
    lib, ctx = _lib.load(), K.context(0)
    ins = [MC.build("saturation", N, C), MC.build("random", N, C)]
    for rows in (16, 64):
        K.set_rows_per_tile(rows)
        assert _gated(N, C, ins, rounds=1) == [KID_LAYER]
        x, base = ins[0]
        assert _plain(x, base, 1, True, f"rows per tile {rows}") == ([KID_C], [KID_D])
    K.set_rows_per_tile(0)
    assert lib.cfx_set_gated_launch(ctx, 0) == 0
    assert _gated(N, C, ins, rounds=2) == [KID_C, KID_D]


# ---- flags, aliasing, base NULL at every shape -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C", MC.SHAPES, ids=[f"{n}x{c}" for n, c in MC.SHAPES])
def test_plain_flags(N, C):
    from compactfusion_amd import codecs as K
    x, base = MC.build("random", N, C, seed=3)
    pkt_ref, nb_ref = oracle(x, base)
    xd, bd = dev(x), dev(base)
    pkt2, nb2 = K.compress(CID, xd, bd, N, C, 0, update_cache=False)
    torch.cuda.synchronize()
    assert nb2 is None
    same_packet(host(pkt2), pkt_ref, "packet (update_cache off)")
    same(host(bd), R.bits(base), "state untouched (update_cache off)")
    pkt3, nb3 = K.compress(CID, xd, bd, N, C, 0, update_cache=True, ef=False)
    torch.cuda.synchronize()
    same_packet(host(pkt3), pkt_ref, "packet (ef off)")
    same(host(nb3), x.view(np.uint16), "state (ef off) == x")
    rec = K.decompress(CID, pkt3, bd, N, C, 0)                         # out of place
    torch.cuda.synchronize()
    same(host(rec), nb_ref, "receiver reconstruction (out of place)")
    peer = bd.clone()
    K.decompress_batch(CID, [pkt3], [peer], [peer], N, C, 0)           # in place
    pk4 = torch.zeros_like(pkt3)
    K.compress_batch(CID, [xd], [bd], [bd], [pk4], N, C, 0, update_cache=True)      # in place
    torch.cuda.synchronize()
    same_packet(host(pk4), pkt_ref, "packet (in place)")
    same(host(bd), nb_ref, "sender state (in place)")
    same(host(peer), nb_ref, "receiver state (in place)")
    # base NULL: the codec sees x itself
    p0_ref, r0_ref = oracle(x, None)
    p0, n0 = K.compress(CID, xd, None, N, C, 0, update_cache=True)
    rec0 = K.decompress(CID, p0, None, N, C, 0)
    torch.cuda.synchronize()
    same_packet(host(p0), p0_ref, "packet (base NULL)")
    same(host(n0), r0_ref, "state (base NULL) == recv")
    same(host(rec0), r0_ref, "reconstruction (base NULL)")


@pytest.mark.parametrize("B", [1, 2, 16])
@pytest.mark.parametrize("N,C", [(3, 64), (5, 320), (17, 576)])
def test_batches(N, C, B):
    from compactfusion_amd import _lib, codecs as K
    lib, ctx = _lib.load(), K.context(0)
    ins = [MC.build("random", N, C, seed=100 * B + i) for i in range(B)]
    refs = [oracle(x, b) for x, b in ins]
    xs = [dev(x) for x, _ in ins]
    bs = [dev(b) for _, b in ins]
    nbs = [torch.empty_like(b) for b in bs]
    pks = [torch.zeros(K.packet_halves(CID, N, C, 0), dtype=torch.float16, device="cuda") for _ in range(B)]
    recs = [torch.empty_like(b) for b in bs]
    ic = _profile(ctx, lib, lambda: K.compress_batch(CID, xs, bs, nbs, pks, N, C, 0, update_cache=True))
    idd = _profile(ctx, lib, lambda: K.decompress_batch(CID, pks, bs, recs, N, C, 0))
    assert ic == [KID_C] and idd == [KID_D], (ic, idd)
    for i, (p_ref, n_ref) in enumerate(refs):
        same_packet(host(pks[i]), p_ref, f"packet item {i}/{B}")
        same(host(nbs[i]), n_ref, f"sender state item {i}/{B}")
        same(host(recs[i]), n_ref, f"reconstruction item {i}/{B}")
        F.check(ins[i][0], ins[i][1], host(pks[i]), host(nbs[i]))
    assert lib.cfx_gate_errors(ctx) == 0


# ---- plan ops --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["compress+decompress", "exchange_layer", "p2p_layer"])
@pytest.mark.parametrize("N,C", [(5, 320), (32, 128), (8, 1024)])
def test_plan_ops(N, C, op):
    """compress + decompress ops; the exchange-layer op without a communicator; the peer-to-peer exchange-layer op looped back in one
    process - two steps each, against the contract"""
    from compactfusion_amd import _lib, codecs as K
    lib, ctx = _lib.load(), K.context(0)
    B, NP = 2, 4
    ins = [MC.build("random", N, C, seed=40 + i) for i in range(B)]
    xd = [dev(x) for x, _ in ins]
    own = [dev(b) for _, b in ins]
    peer = [dev(ins[g % B][1]) for g in range(NP)]
    slot = (K.packet_bytes(CID, N, C, 0) + 255) // 256 * 256
    pk = torch.zeros(B, slot, dtype=torch.uint8, device="cuda")
    comp = (_lib.CompItem * B)(*[_lib.CompItem(xd[i].data_ptr(), own[i].data_ptr(), own[i].data_ptr(), pk[i].data_ptr()) for i in range(B)])
    rec = (_lib.DecompItem * NP)(*[_lib.DecompItem(pk[g % B].data_ptr(), peer[g].data_ptr(), peer[g].data_ptr()) for g in range(NP)])
    plan = lib.cfx_plan_create(ctx)
    flag = torch.zeros(64, dtype=torch.int32, device="cuda")
    if op == "compress+decompress":
        assert lib.cfx_plan_add_compress(plan, CID, N, C, 0, _lib.FLAG_UPDATE_CACHE, B, comp, None, 0) == 0
        assert lib.cfx_plan_add_decompress(plan, CID, N, C, 0, NP, rec) == 1
        n_ops = 2
    elif op == "exchange_layer":
        rc = lib.cfx_plan_add_exchange_layer(plan, CID, N, C, 0, _lib.FLAG_UPDATE_CACHE, B, comp, NP, rec, None, None, None, 0, None, 0)
        assert rc == 0, lib.cfx_last_error_string(ctx)
        n_ops = 1
    else:
        rc = lib.cfx_plan_add_exchange_layer_p2p(plan, CID, N, C, 0, _lib.FLAG_UPDATE_CACHE, B, comp, NP, rec, flag.data_ptr(), 0,
                                                 (ctypes.c_void_p * 1)(), None, 0)
        assert rc == 0, lib.cfx_last_error_string(ctx)
        n_ops = 1
    assert lib.cfx_plan_finalize(plan) == 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    want = [np.ascontiguousarray(b).copy() for _, b in ins]
    nbytes = K.packet_bytes(CID, N, C, 0)
    for step in range(2):
        def run():
            assert lib.cfx_plan_run(plan, 0, n_ops, side.cuda_stream) == 0, lib.cfx_last_error_string(ctx)
        ids = _profile(ctx, lib, run)
        assert lib.cfx_gate_errors(ctx) == 0
        if op == "compress+decompress":
            assert ids == [KID_C, KID_D], (op, ids)
        else:                                               # ONE codec launch: no stand-alone compress or reconstruction behind it
            assert ids.count(KID_LAYER) == 1 and KID_C not in ids and KID_D not in ids, (op, ids)
        for i in range(B):
            p_ref, nb = oracle(ins[i][0], want[i])
            want[i] = nb.view(F16).reshape(N, C)
            same_packet(pk[i, :nbytes].cpu().numpy().view(np.uint16), p_ref, f"{op} step {step}: packet {i}")
            same(host(own[i]), R.bits(want[i]), f"{op} step {step}: sender state {i}")
        for g in range(NP):
            same(host(peer[g]), R.bits(want[g % B]), f"{op} step {step}: peer state {g}")
    lib.cfx_plan_destroy(plan)


# ---- graph capture: the layer call and the p2p layer op, replayed between eager launches ----------------------------------------------
@pytest.mark.parametrize("op", ["gated", "p2p_layer"])
@pytest.mark.parametrize("N,C", [(8, 1024), (32, 128)])
def test_layer_calls_are_graph_capturable(N, C, op):
    """What tests/test_gpu_api.py::test_layer_calls_are_graph_capturable demands of the other codecs: outside a capture the call is ONE
    launch; a capturing stream gets compress ; reconstruct in stream order from the same call.  Four replays with fresh activations,
    eager layer launches before and between them: packets' consequences - sender and peer states - == the contract after every replay."""
    from compactfusion_amd import _lib, codecs as K
    lib, ctx = _lib.load(), K.context(0)
    B, NP = 2, 4
    rng = np.random.default_rng(77 + N)

    def fresh():
        return [(rng.standard_normal((N, C)) * 0.5).astype(F16) for _ in range(B)]
    base = fresh()
    xin = [dev(b) for b in base]
    own = [dev(b) for b in base]
    peer = [dev(base[g % B]) for g in range(NP)]
    want = [b.copy() for b in base]
    slot = (K.packet_bytes(CID, N, C, 0) + 255) // 256 * 256
    pk = torch.zeros(B, slot, dtype=torch.uint8, device="cuda")
    comp = (_lib.CompItem * B)(*[_lib.CompItem(xin[i].data_ptr(), own[i].data_ptr(), own[i].data_ptr(), pk[i].data_ptr()) for i in range(B)])
    gated = (_lib.DecompItem * NP)(*[_lib.DecompItem(pk[g % B].data_ptr(), peer[g].data_ptr(), peer[g].data_ptr()) for g in range(NP)])
    side = torch.cuda.Stream()
    plan = None
    if op == "p2p_layer":
        flag = torch.zeros(64, dtype=torch.int32, device="cuda")
        plan = lib.cfx_plan_create(ctx)
        rc = lib.cfx_plan_add_exchange_layer_p2p(plan, CID, N, C, 0, _lib.FLAG_UPDATE_CACHE, B, comp, NP, gated, flag.data_ptr(), 0,
                                                 (ctypes.c_void_p * 1)(), None, 0)
        assert rc >= 0 and lib.cfx_plan_finalize(plan) == 0, lib.cfx_last_error_string(ctx)

    def call(sh):
        if op == "gated":
            rc = lib.cfx_compress_batch_gated(ctx, CID, N, C, 0, _lib.FLAG_UPDATE_CACHE, B, comp, 0, None, NP, gated, None, 0, sh)
        else:
            rc = lib.cfx_plan_run(plan, 0, 1, sh)
        assert rc == 0, lib.cfx_last_error_string(ctx)

    def step(xs):
        for i in range(B):
            xin[i].copy_(dev(xs[i]))
            _, nb = oracle(xs[i], want[i])
            want[i] = nb.view(F16).reshape(N, C)

    def check(what):
        torch.cuda.synchronize()
        assert lib.cfx_gate_errors(ctx) == 0, what
        for i in range(B):
            same(host(own[i]), R.bits(want[i]), f"{what}: sender state {i}")
        for g in range(NP):
            same(host(peer[g]), R.bits(want[g % B]), f"{what}: peer state {g}")
    step(fresh())
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ids = _profile(ctx, lib, lambda: call(side.cuda_stream))
    assert ids == [KID_LAYER], ids
    check("eager launch before the capture")
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            call(side.cuda_stream)
    torch.cuda.synchronize()
    check("capture must not execute")
    for rep in range(4):
        step(fresh())
        torch.cuda.synchronize()
        graph.replay()
        check(f"replay {rep}")
        if rep == 1:
            step(fresh())
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                call(side.cuda_stream)
            check("eager launch between replays")
    if plan is not None:
        lib.cfx_plan_destroy(plan)


# ---- the stand-alone quantiser pair and the host state machine on the real kernels ----------------------------------------------------
def test_quantize_dequantize_pair():
    from compactfusion_amd.compact import compress_quantize as Q
    N, C = 64, 256
    torch.manual_seed(42)
    d = torch.randn(N, C).half()
    codes, scales = Q.quantize_mxfp4(d.cuda())
    want_pkt, want_recv = M.compress(host(d).reshape(N, C), None)
    by = want_pkt.view(np.uint8)
    assert codes.shape == (N, C // 2) and np.array_equal(codes.cpu().numpy().reshape(-1), by[:N * C // 2])
    assert scales.shape == (N, C // 32) and np.array_equal(scales.cpu().numpy().reshape(-1), by[N * C // 2:])
    same(host(Q.dequantize_mxfp4(codes, scales)), R.bits(want_recv), "dequantize_mxfp4")
    same(host(Q.sim_mxfp4(d.cuda())), R.bits(want_recv), "sim_mxfp4")


def _modes():
    from test_mxfp4_host import MODES
    return MODES


@pytest.mark.parametrize("mode,kw,nwarm", _modes(), ids=[m[0] for m in _modes()])
def test_state_machine_on_the_kernels(mode, kw, nwarm, tmp_path):
    """compact_compress / compact_decompress with MXFP4: residual 1 with error feedback on and off, residual 0, residual 2 (the composition
    around the codec) against R.OracleCompact over the contract, bit for bit"""
    import compactfusion_amd.compact.main as cm
    from compactfusion_amd.collector import collector
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig
    from test_mxfp4_host import _Oracle
    collector.init(collector.Collector(str(tmp_path), enabled=False))
    N, C = 64, 1024
    cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: None, **kw))
    orc_s = _Oracle(residual=kw["residual"], ef=kw["ef"], decay=kw.get("delta_decay_factor"))
    orc_r = _Oracle(residual=kw["residual"], ef=kw["ef"], decay=kw.get("delta_decay_factor"))
    skey, rkey = "0-0-k", "0-1-k"
    for t, x in enumerate(W.drift(11, (N, C), 5)):
        x4 = x.view(1, N, 8, C // 8)
        warm = t < nwarm
        typ, name = (T.WARMUP, "warmup") if warm else (T.MXFP4, "mxfp4")
        pkt = cm.compact_compress(skey, x4.cuda(), typ, update_cache=True)
        want = orc_s.compress(skey, host(x4).reshape(1, N, 8, C // 8), name, True)
        same(host(pkt).reshape(-1), want, f"{mode} step {t}: packet")
        rec = cm.compact_decompress(rkey, pkt.clone(), typ, x4.shape, update_cache=True)
        wrec = orc_r.decompress(rkey, want, name, x4.shape, True)
        same(host(rec).reshape(-1), R.bits(wrec).reshape(-1), f"{mode} step {t}: reconstruction")
        if kw["residual"]:
            same(host(cm.compact_cache().get_base(skey)).reshape(-1), R.bits(orc_s.base[skey]).reshape(-1), f"{mode} step {t}: sender state")
            same(host(cm.compact_cache().get_base(rkey)).reshape(-1), R.bits(orc_r.base[rkey]).reshape(-1), f"{mode} step {t}: receiver state")
        if kw["residual"] == 2 and t >= 1:
            same(host(cm.compact_cache().get_delta_base(skey)).reshape(-1), R.bits(orc_s.dbase[skey]).reshape(-1), f"{mode} step {t}: delta state")
    cm.compact_reset()


# ---- the exchange-layer op with looped-back peers: compact_fwd (ring gather schedule) and compact_all_gather_kv, lane off -------------
from test_gpu_plugin_path import WL, _kernel_ids, loop8      # noqa: E402,F401  (the 8-logical-rank loop-back fixture)


def _replay(seqs, N, C, ef=True):
    """(owner states, peer states) per step: WARMUP, then the contract's residual compress (without error feedback the owner keeps x, a
    peer its reconstruction)"""
    own = seqs[0].numpy().reshape(N, C).copy()
    peer = own.copy()
    outs = [(R.bits(own).copy(), R.bits(peer).copy())]
    for x in seqs[1:]:
        x2 = x.numpy().reshape(N, C)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            pkt, nb = M.residual_compress(x2, own, ef)
            peer = M.residual_decompress(pkt, peer, N, C)
        own = nb
        outs.append((R.bits(own).copy(), R.bits(peer).copy()))
    return outs


@pytest.mark.parametrize("ef", [True, False], ids=["ef", "noef"])
@pytest.mark.parametrize("api", ["ring", "gather"])
def test_plugin_call_one_layer_launch_per_layer(loop8, api, ef):
    """MXFP4 through compact_fwd / compact_all_gather_kv with the lane off: ONE native op per layer, and that op is ONE codec launch
    (kernel id 31: k_mx_layer with the peer-to-peer exchange inside) - no stand-alone compress (13) or decompress (14) launch; 3 steps
    after the warm-up, every logical rank's state against the contract's replay bit for bit"""
    ring, cm, xlayer = loop8
    from compactfusion_amd import _lib, codecs as K
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig, PatchConfig
    lib, ctx = _lib.load(), K.context(0)
    L, STEPS = 2, 4
    shape, N, C = (1, 64, 16, 64), 64, 1024
    kw = dict(enabled=True, compress_func=lambda l, s: T.WARMUP if s == 0 else T.MXFP4, comp_rank=-1, residual=1, ef=ef, fastpath=False)
    if api == "gather":
        kw.update(override_with_patch_gather_fwd=True, patch_gather_fwd_config=PatchConfig(True, False, 1))
    cm.compact_init(CompactConfig(**kw))
    qs = [W.drift(7 + l, shape, STEPS) for l in range(L)]
    ks = [W.drift(17 + l, shape, STEPS) for l in range(L)]
    vs = [W.drift(27 + l, shape, STEPS) for l in range(L)]
    # (the gather keeps every rank's shard - this rank's own too - as a reconstruction: state + decoded packet, whatever error_feedback says)
    efx = ef or api == "gather"
    want = {(l, n): _replay(seq[l], N, C, efx) for l in range(L) for n, seq in (("k", ks), ("v", vs))}
    dev0 = torch.device("cuda:0")
    with torch.cuda.stream(torch.cuda.Stream(dev0)):
        for s in range(STEPS):
            cm.compact_set_step(s)
            torch.cuda.synchronize()
            assert lib.cfx_profile_enable(ctx, 8192, 0xffffffff, 1) == 0
            for l in range(L):
                ring.compact_fwd(qs[l][s].to(dev0), ks[l][s].to(dev0), vs[l][s].to(dev0), causal=False, mod_idx=l, current_iter=s)
            torch.cuda.synchronize()
            got = _kernel_ids(lib, ctx)
            lib.cfx_profile_enable(ctx, 0, 0, 1)
            if s > 0:
                assert got.count(KID_LAYER) == L and not got.count(KID_C) and not got.count(KID_D), (api, s, got)
            cache = cm.compact_cache()
            for l in range(L):
                for n in ("k", "v"):
                    for r in range(WL):
                        key = f"{l}-{r}-{n}" if api == "ring" else f"{l}-{n}-{r}"
                        w = want[(l, n)][s][0 if (r == 0 or efx) else 1]
                        assert np.array_equal(host(cache.get_base(key)).reshape(N, C), w.reshape(N, C)), (api, s, l, n, r)
    ops = [e.xop for e in ring._xbuf.values() if e.xop is not None] + [e.xop for e in cm._kv_exchanges.values() if e.xop is not None]
    assert len(ops) == L and all(o.transport == "p2p" for o in ops), "the layer op / the IPC arena was not used"
    assert lib.cfx_gate_errors(ctx) == 0


# ---- compact_fwd with the exchange lane ON (the default): the layer's chain on the CU-masked lane beside the attention blocks ----------
from test_gpu_lane import W as LW, _late, loopback      # noqa: E402,F401  (the 8-logical-rank ring over the loop-back collective)


@pytest.mark.parametrize("ef", [True, False], ids=["ef", "noef"])
def test_lane_ring_forward(loopback, monkeypatch, ef):
    """compact_fwd at its default settings ("auto": it forks to the lane and joins back) with MXFP4 - on the lane k_mx_decompress publishes
    the chain's flags as k_topk_decompress does -: the owner's and every peer's state against the contract's replay bit for bit, 3 steps
    after the warm-up, the lane plan engaged, no gate error"""
    ring, cm = loopback
    from compactfusion_amd import _lib, codecs as K
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig
    monkeypatch.delenv("CFX_RING_EXCHANGE_STREAM", raising=False)
    monkeypatch.setenv("CFX_LANE", "auto")
    L, STEPS = 3, 4
    shape, N, C = (1, 64, 8, 64), 64, 512
    cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: T.WARMUP if s == 0 else T.MXFP4, comp_rank=-1,
                                  residual=1, ef=ef, fastpath=False))
    qs = [W.drift(7 + l, shape, STEPS) for l in range(L)]
    ks = [W.drift(17 + l, shape, STEPS) for l in range(L)]
    vs = [W.drift(27 + l, shape, STEPS) for l in range(L)]
    want = {(l, n): _replay(seq[l], N, C, ef) for l in range(L) for n, seq in (("k", ks), ("v", vs))}
    dev0 = torch.device("cuda:0")
    stream = torch.cuda.default_stream(dev0)
    with torch.cuda.stream(stream):
        dq, dk, dv = ([[t.to(dev0) for t in seq[l]] for l in range(L)] for seq in (qs, ks, vs))
        for s in range(STEPS):
            cm.compact_set_step(s)
            for l in range(L):
                ring.compact_fwd(dq[l][s], _late(dk[l][s]), _late(dv[l][s]), causal=False, mod_idx=l, current_iter=s)
                assert torch.cuda.current_stream(dev0).cuda_stream == stream.cuda_stream, "the caller's stream is the current stream again"
            torch.cuda.synchronize()
            cache = cm.compact_cache()
            for l in range(L):
                for n in ("k", "v"):
                    for r in range(LW):
                        w = want[(l, n)][s][0 if (r == 0 or ef) else 1]
                        assert np.array_equal(host(cache.get_base(f"{l}-{r}-{n}")).reshape(N, C), w.reshape(N, C)), (s, l, n, r)
    exs = [e for e in ring._xbuf.values() if e.sig is not None]
    assert exs and all(e.lane for e in exs), "the native per-layer lane plan was not used"
    assert len(ring._steady) == L, "the steady-state lane never engaged"
    assert _lib.load().cfx_gate_errors(K.context(0)) == 0


# ---- two rank processes on one GPU through the peer-to-peer transport -----------------------------------------------------------------
def test_p2p_exchange_layer_two_processes_one_gpu(tmp_path):
    """cfx_plan_add_exchange_layer_p2p with codec 8: each rank's packets in memory the other has opened, the exchange inside k_mx_layer
    (remote packets read with system-scope loads).  Three steps; STATES only: every rank's reconstruction of the other's shard is that
    rank's own state, and both are the contract's replay.  Each rank is a fresh process under its own `timeout`; the parent stops at the
    first non-zero exit."""
    Wn, N, C, steps = 2, 33, 128, 3
    env = dict(os.environ)
    env.setdefault("GPU_MAX_HW_QUEUES", "8")
    procs = [subprocess.Popen(["timeout", "-k", "10", "120", sys.executable, os.path.join(HERE, "mxfp4_p2p_rank.py"), str(r), str(Wn), str(tmp_path),
                               str(N), str(C), str(steps)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=REPO, env=env)
             for r in range(Wn)]
    outs = []
    for i, p in enumerate(procs):
        o, _ = p.communicate()
        outs.append(o)
        if p.returncode != 0:
            for q in procs[i + 1:]:
                q.kill()
                q.communicate()
            pytest.fail(f"rank {i} exited with {p.returncode}:\n{o[-2000:]}")
    for r in range(Wn):
        own = np.load(tmp_path / f"own{r}.npy")
        x0 = np.load(tmp_path / f"x0_{r}.npy")
        assert not np.array_equal(own, x0)
        got = np.load(tmp_path / f"peer{1 - r}_{r}.npy")
        assert np.array_equal(got, own), f"rank {1 - r}: reconstruction of rank {r}'s shard differs from rank {r}'s own state"
        xs = [np.load(tmp_path / f"xs{s}_{r}.npy") for s in range(2)]
        st = x0.copy()
        for l in range(st.shape[0]):
            for b in range(2):
                s_ = st[l, b].reshape(N, C)
                for i in range(steps):
                    s_ = oracle(xs[i & 1][l, b].reshape(N, C), s_.view(F16))[1]
                st[l, b] = s_.reshape(st[l, b].shape)
        assert np.array_equal(own, st), f"rank {r}: states differ from the contract's replay"
