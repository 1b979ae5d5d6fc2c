"""The MXINT8 wire codec (id 16) on the GPU (-m gpu), in every launch form, for fp16 and bf16 activations, over its shape and value domain
(tests/_mxint8_cases.py): packets as whole byte strings, sender state, receiver reconstruction and peer states against the numpy contract
(tests/mxint8_contract.py) bit for bit - a state of a 0xFF block is a NaN where the contract's is -, the packet and the sender state against
the independent witness (tests/_mxint8_f64_check.py) as well, no gate error, and every form PROVED by the kernel ids the call launched
(cfx_profile_enable): the stand-alone kernels report top-k's ids 13 / 14, the one-launch layer k_mxi8_layer id 31 - never an abs-mean or
min/max id.

Forms: cfx_compress_batch / cfx_decompress_batch at batch 1, 2, 16; cfx_compress_batch_gated with loop-back peers (31 alone), the same on a
CU-masked stream below 128 CUs and with cfx_set_gated_launch(0) (13, 14); in place and out of place, CFX_FLAG_NO_EF, base NULL; plan ops;
a captured graph of the layer call and of the p2p layer op; compact_fwd / compact_all_gather_kv with the lane off and on; two rank
processes on one GPU.  Every one of them fails where cfx_packet_bytes(16, ...) is 0."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _mxint8_cases as BK
import _mxint8_f64_check as F
import _dist_workers as W
import mxint8_contract as M
from _gpu_codec import KID_LAYER, _profile, host

pytestmark = pytest.mark.gpu

CID = M.CID
KID_C, KID_D = 13, 14            # csrc/cfx_internal.h KID_TOPK_COMPRESS / _DECOMPRESS: what k_mxi8_compress / k_mxi8_decompress report
# csrc/cfx_internal.h: the abs-mean and min/max families' statistics, quantise, dequantise, error-feedback, pipeline and compress launches
OTHER_CODEC_IDS = set(range(1, 13)) | {16, 23, 24, 27, 28, 29}
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
ELEMS = [False, True]
EID = ["fp16", "bf16"]


def dev(u16, bf):
    t = torch.from_numpy(np.ascontiguousarray(u16).view(np.int16))
    return t.view(torch.bfloat16 if bf else torch.float16).cuda()


def same(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, what
    bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} halves differ (first at {int(np.argmax(bad))})"


def same_state(got, want, what, bf):
    """bits; a NaN where the contract has a NaN (the states of a 0xFF block: the contract fixes recv's bits, not a NaN sum's)"""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, what
    lim = 0x7F80 if bf else 0x7C00
    nan = (want & 0x7FFF) > lim
    assert ((got[nan] & 0x7FFF) > lim).all(), f"{what}: not NaN where the contract has NaN"
    same(got[~nan], want[~nan], what)


@pytest.fixture(autouse=True)
def _defaults():
    yield
    from compactfusion_amd import _lib, codecs as K
    assert _lib.load().cfx_set_gated_launch(K.context(0), 1) == 0


def _plain(x, base, bf, rounds, what, f64=True):
    """compress + decompress over `rounds` rounds of error feedback; the kernel ids of the first compress and decompress"""
    from compactfusion_amd import _lib, codecs as K
    lib, ctx = _lib.load(), K.context(0)
    N, C = x.shape
    xd = dev(x, bf)
    bd = None if base is None else dev(base, bf)
    state, ids = base, None
    for t in range(rounds):
        pkt_ref, nb_ref = M.step(x, state, bf)
        out = {}

        def comp():
            out["pkt"], out["nb"] = K.compress(CID, xd, bd, N, C, update_cache=True)

        def dec():
            rec = torch.empty((N, C), dtype=xd.dtype, device="cuda")
            out["rec"] = K.decompress(CID, out["pkt"], bd, N, C, recon=rec)
        if ids is None:
            ids = (_profile(ctx, lib, comp), _profile(ctx, lib, dec))
        else:
            comp()
            dec()
        torch.cuda.synchronize()
        hp, hn = host(out["pkt"]), host(out["nb"]).reshape(N, C)
        same(hp, pkt_ref, f"{what}: packet round {t}")
        same_state(hn, nb_ref, f"{what}: sender state round {t}", bf)
        same_state(host(out["rec"]), nb_ref, f"{what}: receiver reconstruction round {t}", bf)
        if f64:
            F.check(x, state, hp, hn, bf16=bf)
        bd, state = out["nb"], nb_ref.reshape(N, C)
    assert lib.cfx_gate_errors(ctx) == 0
    return ids


def _gated(N, C, bf, ins, rounds, f64=False, NP=3, stream=None):
    """cfx_compress_batch_gated with own error feedback and looped-back peers over rounds, against the contract; the kernel ids of the
    first round.  stream: a raw stream handle (a CU-masked stream), default the current one."""
    from compactfusion_amd import _lib, codecs as K
    lib, ctx = _lib.load(), K.context(0)
    nb_ = len(ins)
    cabi = CID | (M.ELEM_BF16 if bf else 0)
    xs = [x for x, _ in ins]
    xd = [dev(x, bf) for x in xs]
    own = [dev(b, bf) for _, b in ins]
    src = [i % nb_ for i in range(NP)]
    peer = [dev(ins[src[g]][1], bf) for g in range(NP)]
    pk = [torch.zeros(K.packet_halves(CID, N, C), dtype=torch.float16, device="cuda") for _ in range(nb_)]
    sh = torch.cuda.current_stream().cuda_stream if stream is None else stream
    comp = (_lib.CompItem * nb_)(*[_lib.CompItem(xd[i].data_ptr(), own[i].data_ptr(), own[i].data_ptr(), pk[i].data_ptr()) for i in range(nb_)])
    gated = (_lib.DecompItem * NP)(*[_lib.DecompItem(pk[src[g]].data_ptr(), peer[g].data_ptr(), peer[g].data_ptr()) for g in range(NP)])
    torch.cuda.synchronize()

    def go():
        assert lib.cfx_compress_batch_gated(ctx, cabi, N, C, 0, _lib.FLAG_UPDATE_CACHE, nb_, comp, 0, None, NP, gated, None, 0, sh) == 0, \
            lib.cfx_last_error_string(ctx)
    ostate = [np.ascontiguousarray(b).copy() for _, b in ins]
    ids = None
    for t in range(rounds):
        if ids is None:
            ids = _profile(ctx, lib, go)
        else:
            go()
        opk, before = [], [s for s in ostate]
        for i in range(nb_):
            p, nb = M.step(xs[i], ostate[i], bf)
            opk.append(p)
            ostate[i] = nb.reshape(N, C).copy()
        torch.cuda.synchronize()
        assert lib.cfx_gate_errors(ctx) == 0
        for i in range(nb_):
            same(host(pk[i]), opk[i], f"packet round {t} item {i}")
            same_state(host(own[i]), ostate[i], f"own state round {t} item {i}", bf)
            if f64:
                F.check(xs[i], before[i], host(pk[i]), host(own[i]).reshape(N, C), bf16=bf)
        for g in range(NP):
            same_state(host(peer[g]), ostate[src[g]], f"peer state round {t} peer {g}", bf)
    torch.cuda.synchronize()
    return ids


# ---- the value domain in the stand-alone and the layer form --------------------------------------------------------------------------
_PARAMS = [(case, N, C, bf) for bf in ELEMS for case in BK.cases_for(bf) for N, C in BK.SHAPES]


def _pid(p):
    case, N, C, bf = p
    return f"{case}-{N}x{C}-{EID[bf]}"


@pytest.mark.parametrize("case,N,C,bf", _PARAMS, ids=[_pid(p) for p in _PARAMS])
def test_value_domain_stand_alone_and_layer(case, N, C, bf):
    reps = BK.reps(case, N, C)
    for rep in range(reps):
        x, base = BK.build(case, N, C, bf, rep=rep)
        ids = _plain(x, base, bf, 2 if rep == 0 else 1, f"{case} rep {rep}")
        assert ids == ([KID_C], [KID_D]), (case, N, C, ids)
        if rep < 3:
            x0, _ = BK.build(case, N, C, bf, rep=rep, nobase=True)
            assert _plain(x0, None, bf, 1, f"{case} rep {rep} base None") == ([KID_C], [KID_D])
    for rep in range(0, reps, 2):
        ins = [BK.build(case, N, C, bf, rep=r % reps) for r in (rep, rep + 1)]
        ids = _gated(N, C, bf, ins, rounds=2 if rep == 0 else 1, f64=True)
        assert ids == [KID_LAYER], (case, N, C, ids)


@pytest.mark.parametrize("bf", ELEMS, ids=EID)
def test_layer_of_16_items_at_the_flux_shard(bf):
    """K, V and 14 peers' tensors of (544, 3072) in one k_mxi8_layer launch: 2 x 204 S workgroups, 14 x 102 D workgroups"""
    N, C = BK.LAYER16
    ins = [BK.build(case, N, C, bf) for case in ("neighbours", "nonfinite")]
    assert _gated(N, C, bf, ins, rounds=2, NP=14) == [KID_LAYER]


@pytest.mark.parametrize("bf", ELEMS, ids=EID)
def test_gated_batch_of_16(bf):
    """CFX_MAX_BATCH own tensors and as many looped-back peers in one layer launch"""
    N, C = 5, 320
    ins = [BK.build("random", N, C, bf, seed=500 + i) for i in range(16)]
    assert _gated(N, C, bf, ins, rounds=2, NP=16, f64=True) == [KID_LAYER]


# ---- the fall-back forms of the gated call: below 128 CUs, the one-launch forms switched off -------------------------------------------
@pytest.mark.parametrize("bf", ELEMS, ids=EID)
@pytest.mark.parametrize("N,C", [(3, 192), (129, 128), (4, 2112)])
def test_gated_call_on_a_masked_stream_falls_back(N, C, bf):
    from compactfusion_amd import _lib, codecs as K
    lib, ctx = _lib.load(), K.context(0)
    h = ctypes.c_void_p()
    assert lib.cfx_stream_create_masked(ctx, 0, 64, ctypes.byref(h)) == 0
    try:
        ins = [BK.build("ties", N, C, bf), BK.build("random", N, C, bf)]
        assert _gated(N, C, bf, ins, rounds=2, stream=h.value) == [KID_C, KID_D]
    finally:
        torch.cuda.synchronize()
        lib.cfx_stream_destroy(ctx, h)


@pytest.mark.parametrize("bf", ELEMS, ids=EID)
@pytest.mark.parametrize("N,C", [(5, 320), (4, 2112)])
def test_gated_launch_off(N, C, bf):
    from compactfusion_amd import _lib, codecs as K
    lib, ctx = _lib.load(), K.context(0)
    ins = [BK.build("saturation", N, C, bf), BK.build("random", N, C, bf)]
    assert _gated(N, C, bf, ins, rounds=1) == [KID_LAYER]
    assert lib.cfx_set_gated_launch(ctx, 0) == 0
    assert _gated(N, C, bf, ins, rounds=2) == [KID_C, KID_D]


# ---- flags, aliasing, base NULL at every shape -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf", ELEMS, ids=EID)
@pytest.mark.parametrize("N,C", BK.SHAPES, ids=[f"{n}x{c}" for n, c in BK.SHAPES])
def test_plain_flags(N, C, bf):
    from compactfusion_amd import codecs as K
    x, base = BK.build("random", N, C, bf, seed=3)
    pkt_ref, nb_ref = M.step(x, base, bf)
    xd, bd = dev(x, bf), dev(base, bf)
    pkt2, nb2 = K.compress(CID, xd, bd, N, C, update_cache=False)
    torch.cuda.synchronize()
    assert nb2 is None
    same(host(pkt2), pkt_ref, "packet (update_cache off)")
    same(host(bd), base, "state untouched (update_cache off)")
    pkt3, nb3 = K.compress(CID, xd, bd, N, C, update_cache=True, ef=False)
    torch.cuda.synchronize()
    same(host(pkt3), pkt_ref, "packet (ef off)")
    same(host(nb3), x, "state (ef off) == x")
    rec = K.decompress(CID, pkt3, bd, N, C)                         # out of place
    torch.cuda.synchronize()
    assert rec.dtype == xd.dtype
    same(host(rec), nb_ref, "receiver reconstruction (out of place)")
    peer = bd.clone()
    K.decompress_batch(CID, [pkt3], [peer], [peer], N, C)           # in place
    pk4 = torch.zeros_like(pkt3)
    K.compress_batch(CID, [xd], [bd], [bd], [pk4], N, C, update_cache=True)      # in place
    torch.cuda.synchronize()
    same(host(pk4), pkt_ref, "packet (in place)")
    same(host(bd), nb_ref, "sender state (in place)")
    same(host(peer), nb_ref, "receiver state (in place)")
    # base NULL: the codec sees x itself
    p0_ref, r0_ref = M.step(x, None, bf)
    p0, n0 = K.compress(CID, xd, None, N, C, update_cache=True)
    rec0 = K.decompress(CID, p0, None, N, C, recon=torch.empty_like(xd))
    torch.cuda.synchronize()
    same(host(p0), p0_ref, "packet (base NULL)")
    same(host(n0), r0_ref, "state (base NULL) == recv")
    same(host(rec0), r0_ref, "reconstruction (base NULL)")
    if bf:
        # a bf16 sender's packet is an fp16 packet: an fp16 receiver adds the same recv to its fp16 state
        st16 = np.random.default_rng(5).standard_normal((N, C)).astype(np.float16).view(np.uint16)
        rec16 = K.decompress(CID, pkt3, dev(st16, False), N, C)
        torch.cuda.synchronize()
        same(host(rec16), M.recon(pkt_ref, st16, N, C, False), "fp16 receiver of a bf16 sender's packet")


@pytest.mark.parametrize("bf", ELEMS, ids=EID)
@pytest.mark.parametrize("nb_", [1, 2, 16])
@pytest.mark.parametrize("N,C", [(1, 64), (5, 320), (129, 128)])
def test_batches(N, C, nb_, bf):
    from compactfusion_amd import _lib, codecs as K
    lib, ctx = _lib.load(), K.context(0)
    ins = [BK.build("random", N, C, bf, seed=100 * nb_ + i) for i in range(nb_)]
    refs = [M.step(x, b, bf) for x, b in ins]
    xs = [dev(x, bf) for x, _ in ins]
    bs = [dev(b, bf) for _, b in ins]
    nbs = [torch.empty_like(b) for b in bs]
    pks = [torch.zeros(K.packet_halves(CID, N, C), dtype=torch.float16, device="cuda") for _ in range(nb_)]
    recs = [torch.empty_like(b) for b in bs]
    ic = _profile(ctx, lib, lambda: K.compress_batch(CID, xs, bs, nbs, pks, N, C, update_cache=True))
    idd = _profile(ctx, lib, lambda: K.decompress_batch(CID, pks, bs, recs, N, C))
    assert ic == [KID_C] and idd == [KID_D], (ic, idd)
    for i, (p_ref, n_ref) in enumerate(refs):
        same(host(pks[i]), p_ref, f"packet item {i}/{nb_}")
        same(host(nbs[i]), n_ref, f"sender state item {i}/{nb_}")
        same(host(recs[i]), n_ref, f"reconstruction item {i}/{nb_}")
        F.check(ins[i][0], ins[i][1], host(pks[i]), host(nbs[i]), bf16=bf)
    assert lib.cfx_gate_errors(ctx) == 0


# ---- plan ops --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf", ELEMS, ids=EID)
@pytest.mark.parametrize("op", ["compress+decompress", "exchange_layer", "p2p_layer"])
@pytest.mark.parametrize("N,C", [(3, 192), (129, 128), (4, 2112)])
def test_plan_ops(N, C, op, bf):
    """compress + decompress ops (added to one plan, run from a copy); the exchange-layer op without a communicator; the peer-to-peer
    exchange-layer op looped back in one process - two steps each, against the contract"""
    from compactfusion_amd import _lib, codecs as K
    lib, ctx = _lib.load(), K.context(0)
    nb_, NP = 2, 4
    cabi = CID | (M.ELEM_BF16 if bf else 0)
    ins = [BK.build("random", N, C, bf, seed=40 + i) for i in range(nb_)]
    xd = [dev(x, bf) for x, _ in ins]
    own = [dev(b, bf) for _, b in ins]
    peer = [dev(ins[g % nb_][1], bf) for g in range(NP)]
    nbytes = K.packet_bytes(cabi, N, C)
    slot = (nbytes + 255) // 256 * 256
    pk = torch.zeros(nb_, slot, dtype=torch.uint8, device="cuda")
    comp = (_lib.CompItem * nb_)(*[_lib.CompItem(xd[i].data_ptr(), own[i].data_ptr(), own[i].data_ptr(), pk[i].data_ptr()) for i in range(nb_)])
    rec = (_lib.DecompItem * NP)(*[_lib.DecompItem(pk[g % nb_].data_ptr(), peer[g].data_ptr(), peer[g].data_ptr()) for g in range(NP)])
    plan = lib.cfx_plan_create(ctx)
    flag = torch.zeros(64, dtype=torch.int32, device="cuda")
    if op == "compress+decompress":
        first = lib.cfx_plan_create(ctx)
        assert lib.cfx_plan_add_compress(first, cabi, N, C, 0, _lib.FLAG_UPDATE_CACHE, nb_, comp, None, 0) == 0
        assert lib.cfx_plan_add_decompress(first, cabi, N, C, 0, NP, rec) == 1
        assert [lib.cfx_plan_copy_op(plan, first, i) for i in range(2)] == [0, 1]
        lib.cfx_plan_destroy(first)
        n_ops = 2
    elif op == "exchange_layer":
        rc = lib.cfx_plan_add_exchange_layer(plan, cabi, N, C, 0, _lib.FLAG_UPDATE_CACHE, nb_, comp, NP, rec, None, None, None, 0, None, 0)
        assert rc == 0, lib.cfx_last_error_string(ctx)
        n_ops = 1
    else:
        rc = lib.cfx_plan_add_exchange_layer_p2p(plan, cabi, N, C, 0, _lib.FLAG_UPDATE_CACHE, nb_, comp, NP, rec, flag.data_ptr(), 0,
                                                 (ctypes.c_void_p * 1)(), None, 0)
        assert rc == 0, lib.cfx_last_error_string(ctx)
        n_ops = 1
    assert lib.cfx_plan_finalize(plan) == 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    want = [np.ascontiguousarray(b).copy() for _, b in ins]
    for step in range(2):
        def run():
            assert lib.cfx_plan_run(plan, 0, n_ops, side.cuda_stream) == 0, lib.cfx_last_error_string(ctx)
        ids = _profile(ctx, lib, run)
        assert lib.cfx_gate_errors(ctx) == 0
        if op == "compress+decompress":
            assert ids == [KID_C, KID_D], (op, ids)
        else:                                               # ONE codec launch: no stand-alone compress or reconstruction behind it
            assert ids.count(KID_LAYER) == 1 and KID_C not in ids and KID_D not in ids and not (set(ids) & OTHER_CODEC_IDS), (op, ids)
        for i in range(nb_):
            p_ref, nb = M.step(ins[i][0], want[i], bf)
            want[i] = nb.reshape(N, C)
            same(pk[i, :nbytes].cpu().numpy().view(np.uint16), p_ref, f"{op} step {step}: packet {i}")
            same(host(own[i]), want[i], f"{op} step {step}: sender state {i}")
        for g in range(NP):
            same(host(peer[g]), want[g % nb_], f"{op} step {step}: peer state {g}")
    lib.cfx_plan_destroy(plan)


# ---- graph capture: the layer call and the p2p layer op, one capture and three replays between eager launches --------------------------
@pytest.mark.parametrize("bf", ELEMS, ids=EID)
@pytest.mark.parametrize("op", ["gated", "p2p_layer"])
@pytest.mark.parametrize("N,C", [(8, 1024), (33, 128)])
def test_layer_calls_are_graph_capturable(N, C, op, bf):
    """Outside a capture the call is ONE launch; a capturing stream gets compress ; reconstruct in stream order from the same call.  Three
    replays with fresh activations, eager layer launches before and between them: sender and peer states == the contract after every one.
    The captured sequence is proved by its results alone, not by kernel ids: the profile (cfx_profile_enable) times a launch with a pair of
    events handed to the launch itself and read once the call has run; under capture nothing runs in the call, and the replay is
    dispatched by the runtime, not through the library - the profile is left off there.  The fall-backs that do run in the call (a
    CU-masked stream, the gated launch switched off) are proved by their ids 13, 14 above."""
    from compactfusion_amd import _lib, codecs as K
    lib, ctx = _lib.load(), K.context(0)
    nb_, NP = 2, 4
    cabi = CID | (M.ELEM_BF16 if bf else 0)
    rng = np.random.default_rng(77 + N)

    def fresh():
        f = [(rng.standard_normal((N, C)) * 0.5).astype(np.float32) for _ in range(nb_)]
        return [M.BC.f32_to_bf16(a) if bf else a.astype(np.float16).view(np.uint16) for a in f]
    base = fresh()
    xin = [dev(b, bf) for b in base]
    own = [dev(b, bf) for b in base]
    peer = [dev(base[g % nb_], bf) for g in range(NP)]
    want = [b.copy() for b in base]
    slot = (K.packet_bytes(cabi, N, C) + 255) // 256 * 256
    pk = torch.zeros(nb_, slot, dtype=torch.uint8, device="cuda")
    comp = (_lib.CompItem * nb_)(*[_lib.CompItem(xin[i].data_ptr(), own[i].data_ptr(), own[i].data_ptr(), pk[i].data_ptr()) for i in range(nb_)])
    gated = (_lib.DecompItem * NP)(*[_lib.DecompItem(pk[g % nb_].data_ptr(), peer[g].data_ptr(), peer[g].data_ptr()) for g in range(NP)])
    side = torch.cuda.Stream()
    plan = None
    if op == "p2p_layer":
        flag = torch.zeros(64, dtype=torch.int32, device="cuda")
        plan = lib.cfx_plan_create(ctx)
        rc = lib.cfx_plan_add_exchange_layer_p2p(plan, cabi, N, C, 0, _lib.FLAG_UPDATE_CACHE, nb_, comp, NP, gated, flag.data_ptr(), 0,
                                                 (ctypes.c_void_p * 1)(), None, 0)
        assert rc >= 0 and lib.cfx_plan_finalize(plan) == 0, lib.cfx_last_error_string(ctx)

    def call(sh):
        if op == "gated":
            rc = lib.cfx_compress_batch_gated(ctx, cabi, N, C, 0, _lib.FLAG_UPDATE_CACHE, nb_, comp, 0, None, NP, gated, None, 0, sh)
        else:
            rc = lib.cfx_plan_run(plan, 0, 1, sh)
        assert rc == 0, lib.cfx_last_error_string(ctx)

    def step(xs):
        for i in range(nb_):
            xin[i].copy_(dev(xs[i], bf))
            want[i] = M.step(xs[i], want[i], bf)[1].reshape(N, C)

    def check(what):
        torch.cuda.synchronize()
        assert lib.cfx_gate_errors(ctx) == 0, what
        for i in range(nb_):
            same(host(own[i]), want[i], f"{what}: sender state {i}")
        for g in range(NP):
            same(host(peer[g]), want[g % nb_], f"{what}: peer state {g}")
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
    for rep in range(3):
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
def test_quantize_dequantize_triple():
    from compactfusion_amd.compact import compress_quantize as Q
    from oracle import ref_np as R
    N, C = 64, 256
    torch.manual_seed(42)
    d = torch.randn(N, C).half()
    codes, scales = Q.quantize_mxint8(d.cuda())
    want_pkt, want_recv = M.compress(host(d).reshape(N, C).view(np.float16), None)
    wq, ws = M.split(want_pkt, N, C)
    assert codes.shape == (N, C) and codes.dtype == torch.int8 and np.array_equal(codes.cpu().numpy(), wq)
    assert scales.shape == (N, C // 32) and scales.dtype == torch.uint8 and np.array_equal(scales.cpu().numpy(), ws)
    same(host(Q.dequantize_mxint8(codes, scales)), R.bits(want_recv), "dequantize_mxint8")
    same(host(Q.sim_mxint8(d.cuda())), R.bits(want_recv), "sim_mxint8")


@pytest.mark.parametrize("bf", ELEMS, ids=EID)
def test_receiver_reads_the_byte_0x80_as_minus_127(bf):
    """a byte no sender writes: the stand-alone reconstruction decodes 0x80 as -127, on a state and with base NULL"""
    from compactfusion_amd import codecs as K
    N, C = 3, 192
    rng = np.random.default_rng(9)
    pkt = np.zeros(M.packet_halves(N, C), dtype=np.uint16)
    by = pkt.view(np.uint8)
    by[:N * C] = rng.integers(0, 256, N * C)
    by[:N * C:7] = 0x80
    by[N * C:] = rng.integers(109, 143, N * C // 32)
    x, base = BK.build("random", N, C, bf, seed=9)
    pd = torch.from_numpy(pkt.view(np.int16)).view(torch.float16).cuda()
    rec = K.decompress(CID, pd, dev(base, bf), N, C)
    rec0 = K.decompress(CID, pd, None, N, C, recon=torch.empty_like(rec))
    torch.cuda.synchronize()
    same(host(rec), M.recon(pkt, base, N, C, bf), "reconstruction on a state")
    same(host(rec0), M.recon(pkt, None, N, C, bf), "reconstruction with base NULL")
    assert (M.split(pkt, N, C)[0] == -128).sum() >= N * C // 7


_SM = [("res1_ef", dict(residual=1, ef=True), False), ("res1_ef", dict(residual=1, ef=True), True),
       ("res1_noef", dict(residual=1, ef=False), True), ("res0", dict(residual=0, ef=False), False),
       ("res0", dict(residual=0, ef=False), True)]


@pytest.mark.parametrize("mode,kw,bf", _SM, ids=[f"{m}-{EID[bf]}" for m, _, bf in _SM])
def test_state_machine_on_the_kernels(mode, kw, bf, tmp_path):
    """compact_compress / compact_decompress with MXINT8: residual 1 with error feedback on and off,
    residual 0, fp16 and bf16, against the contract bit for bit"""
    import compactfusion_amd.compact.main as cm
    from compactfusion_amd import config
    from compactfusion_amd.collector import collector
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig
    collector.init(collector.Collector(str(tmp_path), enabled=False))
    N, C = 64, 1024
    dt = torch.bfloat16 if bf else torch.float16
    try:
        cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: None, **kw))
        res, ef = kw["residual"], kw["ef"]
        skey, rkey = "0-0-k", "0-1-k"
        s_state = r_state = None
        for t, x in enumerate(W.drift(11, (N, C), 5)):
            x4 = x.to(dt).view(1, N, 8, C // 8)
            xb = host(x4).reshape(N, C)
            warm = res == 1 and t == 0
            typ = T.WARMUP if warm else T.MXINT8
            pkt = cm.compact_compress(skey, x4.cuda(), typ, update_cache=True)
            if warm:
                cm.compact_decompress(rkey, pkt.clone(), typ, x4.shape, update_cache=True)
                s_state, r_state = xb.copy(), xb.copy()
                continue
            want_pkt, nb = M.step(xb, s_state if res else None, bf, ef)
            same(host(pkt).reshape(-1), want_pkt, f"{mode} step {t}: packet")
            want_rec = M.recon(want_pkt, r_state if res else None, N, C, bf)
            rec = cm._decompress(rkey, pkt.clone(), typ, x4.shape, True, dt)
            assert rec.dtype == dt
            same(host(rec).reshape(-1), want_rec, f"{mode} step {t}: reconstruction")
            if res:
                s_state, r_state = nb.reshape(N, C), want_rec.reshape(N, C)
                same(host(cm.compact_cache().get_base(skey)).reshape(-1), s_state, f"{mode} step {t}: sender state")
                same(host(cm.compact_cache().get_base(rkey)).reshape(-1), r_state, f"{mode} step {t}: receiver state")
    finally:
        cm.compact_reset()
        config.reset()


def test_residual_2_on_the_kernels(tmp_path):
    """fp16, residual 2: the composition around the codec against R.OracleCompact over the contract, bit for bit"""
    import compactfusion_amd.compact.main as cm
    from compactfusion_amd import config
    from compactfusion_amd.collector import collector
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig
    from oracle import ref_np as R
    from test_mxint8_host import _Oracle
    collector.init(collector.Collector(str(tmp_path), enabled=False))
    N, C = 64, 1024
    try:
        cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: None, residual=2, ef=True, delta_decay_factor=0.5))
        orc_s, orc_r = (_Oracle(residual=2, ef=True, decay=0.5) for _ in range(2))
        skey, rkey = "0-0-k", "0-1-k"
        for t, x in enumerate(W.drift(11, (N, C), 5)):
            x4 = x.view(1, N, 8, C // 8)
            warm = t < 2
            typ, name = (T.WARMUP, "warmup") if warm else (T.MXINT8, M.NAME)
            pkt = cm.compact_compress(skey, x4.cuda(), typ, update_cache=True)
            want = orc_s.compress(skey, host(x4).reshape(1, N, 8, C // 8), name, True)
            same(host(pkt).reshape(-1), want, f"step {t}: packet")
            rec = cm.compact_decompress(rkey, pkt.clone(), typ, x4.shape, update_cache=True)
            wrec = orc_r.decompress(rkey, want, name, x4.shape, True)
            same(host(rec).reshape(-1), R.bits(wrec).reshape(-1), f"step {t}: reconstruction")
            same(host(cm.compact_cache().get_base(skey)).reshape(-1), R.bits(orc_s.base[skey]).reshape(-1), f"step {t}: sender state")
            same(host(cm.compact_cache().get_base(rkey)).reshape(-1), R.bits(orc_r.base[rkey]).reshape(-1), f"step {t}: receiver state")
            if t >= 1:
                same(host(cm.compact_cache().get_delta_base(skey)).reshape(-1), R.bits(orc_s.dbase[skey]).reshape(-1), f"step {t}: delta state")
    finally:
        cm.compact_reset()
        config.reset()


# ---- the exchange-layer op with looped-back peers: compact_fwd (ring gather schedule) and compact_all_gather_kv, lane off -------------
from test_gpu_plugin_path import WL, _kernel_ids, loop8      # noqa: E402,F401  (the 8-logical-rank loop-back fixture)


def _replay(seqs, N, C, bf, ef=True):
    """(owner states, peer states) per step: WARMUP, then the contract's residual compress (without error feedback the owner keeps x, a
    peer its reconstruction)"""
    own = host(seqs[0]).reshape(N, C).copy()
    peer = own.copy()
    outs = [(own.copy(), peer.copy())]
    for x in seqs[1:]:
        pkt, nb = M.step(host(x).reshape(N, C), own, bf, ef)
        peer = M.recon(pkt, peer, N, C, bf).reshape(N, C)
        own = nb.reshape(N, C)
        outs.append((own.copy(), peer.copy()))
    return outs


def _drift(seed, shape, steps, bf):
    return [x.bfloat16() if bf else x for x in W.drift(seed, shape, steps)]


@pytest.mark.parametrize("api,ef,bf", [("ring", True, False), ("ring", False, True), ("gather", True, True), ("gather", True, False)],
                         ids=["ring-ef-fp16", "ring-noef-bf16", "gather-bf16", "gather-fp16"])
def test_plugin_call_one_layer_launch_per_layer(loop8, api, ef, bf):
    """MXINT8 through compact_fwd / compact_all_gather_kv with the lane off: ONE native op per layer, and that op is ONE codec launch
    (kernel id 31: k_mxi8_layer with the peer-to-peer exchange inside) - no stand-alone compress (13) or decompress (14) launch, no abs-mean
    id; 3 steps after the warm-up, every logical rank's state against the contract's replay bit for bit"""
    ring, cm, xlayer = loop8
    from compactfusion_amd import _lib, codecs as K, config
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig, PatchConfig
    lib, ctx = _lib.load(), K.context(0)
    L, STEPS = 2, 4
    shape, N, C = (1, 64, 16, 64), 64, 1024
    try:
        kw = dict(enabled=True, compress_func=lambda l, s: T.WARMUP if s == 0 else T.MXINT8, comp_rank=-1, residual=1, ef=ef, fastpath=False)
        if api == "gather":
            kw.update(override_with_patch_gather_fwd=True, patch_gather_fwd_config=PatchConfig(True, False, 1))
        cm.compact_init(CompactConfig(**kw))
        qs = [_drift(7 + l, shape, STEPS, bf) for l in range(L)]
        ks = [_drift(17 + l, shape, STEPS, bf) for l in range(L)]
        vs = [_drift(27 + l, shape, STEPS, bf) for l in range(L)]
        # (the gather keeps every rank's shard - this rank's own too - as a reconstruction: state + decoded packet, whatever error_feedback says)
        efx = ef or api == "gather"
        want = {(l, n): _replay(seq[l], N, C, bf, efx) for l in range(L) for n, seq in (("k", ks), ("v", vs))}
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
                    assert not (set(got) & OTHER_CODEC_IDS), (api, s, got)
                cache = cm.compact_cache()
                for l in range(L):
                    for n in ("k", "v"):
                        for r in range(WL):
                            key = f"{l}-{r}-{n}" if api == "ring" else f"{l}-{n}-{r}"
                            w = want[(l, n)][s][0 if (r == 0 or efx) else 1]
                            st = cache.get_base(key)
                            assert st.dtype == (torch.bfloat16 if bf else torch.float16)
                            assert np.array_equal(host(st).reshape(N, C), w.reshape(N, C)), (api, s, l, n, r)
        ops = [e.xop for e in ring._xbuf.values() if e.xop is not None] + [e.xop for e in cm._kv_exchanges.values() if e.xop is not None]
        assert len(ops) == L and all(o.transport == "p2p" for o in ops), "the layer op / the IPC arena was not used"
        assert lib.cfx_gate_errors(ctx) == 0
    finally:
        config.reset()


# ---- compact_fwd with the exchange lane ON (the default): the layer's chain on the CU-masked lane beside the attention blocks ----------
from test_gpu_lane import W as LW, _late, loopback      # noqa: E402,F401  (the 8-logical-rank ring over the loop-back collective)


@pytest.mark.parametrize("ef,bf", [(True, False), (True, True), (False, True)], ids=["ef-fp16", "ef-bf16", "noef-bf16"])
def test_lane_ring_forward(loopback, monkeypatch, ef, bf):
    """compact_fwd at its default settings ("auto": it forks to the lane and joins back) with MXINT8 - on the lane k_mxi8_decompress
    publishes the chain's flags as k_mx_decompress does -: the owner's and every peer's state against the contract's replay bit for bit,
    3 steps after the warm-up, the lane plan engaged, no gate error"""
    ring, cm = loopback
    from compactfusion_amd import _lib, codecs as K, config
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig
    monkeypatch.delenv("CFX_RING_EXCHANGE_STREAM", raising=False)
    monkeypatch.setenv("CFX_LANE", "auto")
    L, STEPS = 3, 4
    shape, N, C = (1, 64, 8, 64), 64, 512
    try:
        cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: T.WARMUP if s == 0 else T.MXINT8, comp_rank=-1,
                                      residual=1, ef=ef, fastpath=False))
        qs = [_drift(7 + l, shape, STEPS, bf) for l in range(L)]
        ks = [_drift(17 + l, shape, STEPS, bf) for l in range(L)]
        vs = [_drift(27 + l, shape, STEPS, bf) for l in range(L)]
        want = {(l, n): _replay(seq[l], N, C, bf, ef) for l in range(L) for n, seq in (("k", ks), ("v", vs))}
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
    finally:
        config.reset()


# ---- two rank processes on one GPU through the peer-to-peer transport -----------------------------------------------------------------
@pytest.mark.parametrize("bf", ELEMS, ids=EID)
def test_p2p_exchange_layer_two_processes_one_gpu(tmp_path, bf):
    """cfx_plan_add_exchange_layer_p2p with codec 16: each rank's packets in memory the other has opened, the exchange inside k_mxi8_layer
    (remote packets read with system-scope loads).  Three steps; STATES only: every rank's reconstruction of the other's shard is that
    rank's own state, and both are the contract's replay.  Each rank is a fresh process under its own `timeout`; the parent stops at the
    first non-zero exit."""
    Wn, N, C, steps = 2, 33, 128, 3
    env = dict(os.environ)
    env.setdefault("GPU_MAX_HW_QUEUES", "8")
    procs = [subprocess.Popen(["timeout", "-k", "10", "120", sys.executable, os.path.join(HERE, "mxint8_p2p_rank.py"), str(r), str(Wn), str(tmp_path),
                               str(N), str(C), str(steps), str(int(bf))], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                              cwd=REPO, env=env) for r in range(Wn)]
    for i, p in enumerate(procs):
        o, _ = p.communicate()
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
                    s_ = M.step(xs[i & 1][l, b].reshape(N, C), s_, bf)[1].reshape(N, C)
                st[l, b] = s_.reshape(st[l, b].shape)
        assert np.array_equal(own, st), f"rank {r}: states differ from the contract's replay"
