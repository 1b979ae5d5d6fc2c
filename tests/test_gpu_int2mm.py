"""The INT2_MINMAX wire codec (id 6) on the GPU (-m gpu), in every launch form INT4 has, over its shape and value domain
(tests/_int2mm_cases.py).  Packets against the numpy contract (tests/int2mm_contract.py; the `min` half under the signed-zero rule of
tests/_zero_min.py, used on planted channels only), sender state, receiver reconstruction and peer states bit for bit, the float64
definition wherever the case is finite, no gate error - and every form PROVED by the kernel ids the call launched (cfx_profile_enable;
the quantise / dequantise kernels report INT4's ids 11 / 12).

Forms (cfx_i_minmax_compress; FORMS below): the layer launch (kernel id 31 alone; C % 16 == 0) with S tiles of 32 rows or 64, the cooperative
reduce (more than 32 partials a channel), the tall form (more than 64); k_minmax_compress (29; C % 16 == 8, or statistics rows set) with
the quantiser (11) and, gated, the dequantiser (12) behind it; k_minmax_stats + k_minmax_finalize (7, 8; in-launch finalize off) at rows per
tile 0 / 16 / 32 / 64 / 128; batches of 1 and 16; a captured graph; the exchange-layer op with looped-back peers through compact_fwd and
compact_all_gather_kv; two rank processes on one GPU."""
import ctypes

import numpy as np
import pytest
import torch

import _dist_workers as W
import _int2mm_cases as IC
import _zero_min as Z
import int2mm_contract as I
from _gpu_codec import KID_LAYER, _profile, dev, host, inputs, same_bits
from oracle import ref_np as R

pytestmark = pytest.mark.gpu

F16 = np.float16
CID = I.CID
QUANT, DEQUANT, KID_STATS, KID_FINALIZE, KID_MM_COMPRESS = 11, 12, 7, 8, 29

# (form, shapes, in-launch finalize, rows per tile, statistics rows, the layer launch's sub-form or None)
FORMS = [
    ("layer-32-row-tiles", [(68, 144), (68, 528), (132, 144), (516, 192), (544, 576), (4, 1168)], True, 0, 0, "S32"),
    ("layer-64-row-tiles", [(1028, 16)], True, 0, 0, "S64"),
    ("layer-cooperative-reduce", [(2052, 16)], True, 0, 0, "coop"),
    ("layer-tall", [(4100, 16)], True, 0, 0, "tall"),
    ("minmax-compress", [(4, 72), (8, 72), (20, 24), (68, 136), (132, 520)], True, 0, 0, None),
    ("minmax-compress-stats-rows-16", [(68, 144)], True, 0, 16, None),
    ("minmax-compress-stats-rows-64", [(132, 520), (516, 192)], True, 0, 64, None),
    ("stats-finalize-rows-0", [(68, 136), (68, 144)], False, 0, 0, None),
    ("stats-finalize-rows-16", [(68, 136), (68, 144)], False, 16, 0, None),
    ("stats-finalize-rows-32", [(68, 136)], False, 32, 0, None),
    ("stats-finalize-rows-64", [(132, 520)], False, 64, 0, None),
    ("stats-finalize-rows-128", [(68, 136), (516, 192)], False, 128, 0, None),
]


def layer_sub_form(N):
    """cfx_i_minmax_compress: RL, PL, coop, tall (MML_MAX_P = 64)"""
    RL = 32 if (N + 31) // 32 <= 32 else 64
    PL = (N + RL - 1) // RL
    return "tall" if PL > 64 else ("coop" if PL > 32 else f"S{RL}")


def want_ids(form):
    """(plain compress, plain decompress, gated call) kernel ids of a form"""
    if form.startswith("layer"):
        return [KID_LAYER], [DEQUANT], [KID_LAYER]
    if form.startswith("stats-finalize"):
        return [KID_STATS, KID_FINALIZE, QUANT], [DEQUANT], [KID_STATS, KID_FINALIZE, QUANT, DEQUANT]
    return [KID_MM_COMPRESS, QUANT], [DEQUANT], [KID_MM_COMPRESS, QUANT, DEQUANT]


def oracle(x, base, ef=True):
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        pkt, nb = I.residual_compress(x, base, ef)
    return np.asarray(pkt).view(np.uint16), R.bits(nb)


def same_packet(got, want, x, base, what, allowed=None):
    """bit for bit but for the `min` half under the signed-zero rule (include/cfx.h: INT4's rule; tests/_zero_min.py - the packet's last C
    halves are `min` as in INT4's)"""
    used = Z.same_packet("int4", got, want, x, base, what)
    if allowed is None:
        assert not used, f"{what}: min differs by the sign of a zero on channel(s) {sorted(used)[:8]} of an input that plants none"
    else:
        allowed |= used


def _settings(fused, rows, srows):
    from compactfusion_amd import _lib, codecs as K
    K.set_fused_finalize(fused)
    K.set_rows_per_tile(rows)
    assert _lib.load().cfx_set_stats_rows(K.context(0), srows) == 0


@pytest.fixture(autouse=True)
def _defaults():
    yield
    _settings(True, 0, 0)


def _plain(x, base, rounds, finite, allowed, what):
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
        same_packet(hp, pkt_ref, x, state, f"{what}: packet round {t}", allowed)
        same_bits(hn, nb_ref, f"{what}: sender state round {t}")
        same_bits(host(out["rec"]), nb_ref, f"{what}: receiver reconstruction round {t}")
        if finite:
            I.check_f64(x, state, hp, hn)
        bd, state = out["nb"], nb_ref.view(F16).reshape(N, C)
    assert lib.cfx_gate_errors(ctx) == 0
    return ids


def _gated(N, C, ins, rounds, allowed=None, f64=False, check=True, NP=3):
    """cfx_compress_batch_gated with own error feedback and looped-back peers over rounds (as tests/_gpu_codec.py::_gated_layer, against
    the contract); the kernel ids of the first round"""
    from compactfusion_amd import _lib, codecs as K
    lib, ctx = _lib.load(), K.context(0)
    B = len(ins)
    xs = [x for x, _ in ins]
    xd = [dev(x) for x in xs]
    own = [dev(b) for _, b in ins]
    src = [i % B for i in range(NP)]
    peer = [dev(ins[src[g]][1]) for g in range(NP)]
    pk = [torch.zeros(K.packet_halves(CID, N, C, 0), dtype=torch.float16, device="cuda") for _ in range(B)]
    ws = K.workspace(CID, N, C, 0, B, 0)
    sh = torch.cuda.current_stream().cuda_stream
    comp = (_lib.CompItem * B)(*[_lib.CompItem(xd[i].data_ptr(), own[i].data_ptr(), own[i].data_ptr(), pk[i].data_ptr()) for i in range(B)])
    gated = (_lib.DecompItem * NP)(*[_lib.DecompItem(pk[src[g]].data_ptr(), peer[g].data_ptr(), peer[g].data_ptr()) for g in range(NP)])

    def go():
        assert lib.cfx_compress_batch_gated(ctx, CID, N, C, 0, _lib.FLAG_UPDATE_CACHE, B, comp, 0, None, NP, gated, ws.data_ptr(), ws.numel(), sh) == 0
    ostate = [np.ascontiguousarray(b).view(np.uint16).copy() for _, b in ins]
    ids = None
    for t in range(rounds):
        if ids is None:
            ids = _profile(ctx, lib, go)
        else:
            go()
        if not check:
            continue
        opk, before = [], [s for s in ostate]
        for i in range(B):
            p, nb = oracle(xs[i], ostate[i].view(F16))
            opk.append(p)
            ostate[i] = nb.copy()
        torch.cuda.synchronize()
        assert lib.cfx_gate_errors(ctx) == 0
        for i in range(B):
            same_packet(host(pk[i]), opk[i], xs[i], before[i].view(F16), f"packet round {t} item {i}", allowed)
            same_bits(host(own[i]), ostate[i], f"own state round {t} item {i}")
            if f64:
                I.check_f64(xs[i], before[i].view(F16), host(pk[i]), host(own[i]).reshape(N, C))
        for g in range(NP):
            same_bits(host(peer[g]), ostate[src[g]], f"peer state round {t} peer {g}")
    torch.cuda.synchronize()
    return ids


# ---- the value domain in every launch form ---------------------------------------------------------------------------------------------
def _params():
    return [pytest.param(form, fused, rows, srows, sub, N, C, case, id=f"{form}-{N}x{C}-{case}")
            for form, shapes, fused, rows, srows, sub in FORMS for N, C in shapes for case in IC.NAMES]


@pytest.mark.parametrize("form,fused,rows,srows,sub,N,C,case", _params())
def test_value_domain_in_every_launch_form(form, fused, rows, srows, sub, N, C, case):
    assert sub is None or layer_sub_form(N) == sub
    _settings(fused, rows, srows)
    want_c, want_d, want_g = want_ids(form)
    finite = case in IC.FINITE
    allowed = set()
    for rep in range(IC.reps(case, N, C)):
        x, base = IC.build(case, N, C, rep=rep)
        ids = _plain(x, base, 2 if rep == 0 else 1, finite, allowed, f"{case} rep {rep}")
        assert ids == (want_c, want_d), (form, N, C, ids)
    x0, _ = IC.build(case, N, C, nobase=True)
    ids = _plain(x0, None, 1, finite, allowed, f"{case} base None")
    assert ids == (want_c, want_d), (form, N, C, ids)
    ins = [IC.build(case, N, C, rep=r) for r in (0, 1)]
    ids = _gated(N, C, ins, rounds=2, allowed=allowed, f64=finite)
    assert ids == want_g, (form, N, C, ids)
    assert allowed <= IC.signed_zero_channels(case, N, C), f"the signed-zero rule was used on channels {sorted(allowed)} that the case does not plant"


def test_forms_table_covers_every_shape_and_sub_form():
    assert {s for _, shapes, *_ in FORMS for s in shapes} == set(IC.ALL_SHAPES)
    assert {sub for *_, sub in FORMS if sub} == {"S32", "S64", "coop", "tall"}
    for form, shapes, fused, rows, srows, sub in FORMS:
        for N, C in shapes:
            assert N % 4 == 0 and (sub is None) == (C % 16 != 0 or not fused or srows != 0), (form, N, C)
    assert any((N // 4 * C) % 16 for _, shapes, *_ in FORMS for N, C in shapes), "no shape with tail sections off 16 bytes"


# ---- update_cache off, error feedback off, random inputs at every shape ----------------------------------------------------------------
@pytest.mark.parametrize("N,C", IC.ALL_SHAPES, ids=[f"{n}x{c}" for n, c in IC.ALL_SHAPES])
def test_plain_flags(N, C):
    from compactfusion_amd import codecs as K
    x, base = inputs(N * 131 + C, N, C)
    pkt_ref, nb_ref = oracle(x, base)
    xd, bd = dev(x), dev(base)
    pkt2, nb2 = K.compress(CID, xd, bd, N, C, 0, update_cache=False)
    torch.cuda.synchronize()
    assert nb2 is None
    same_packet(host(pkt2), pkt_ref, x, base, "packet (update_cache off)")
    pkt3, nb3 = K.compress(CID, xd, bd, N, C, 0, update_cache=True, ef=False)
    torch.cuda.synchronize()
    same_packet(host(pkt3), pkt_ref, x, base, "packet (ef off)")
    same_bits(host(nb3), x.view(np.uint16), "state (ef off) == x")
    rec = K.decompress(CID, pkt3, bd, N, C, 0)
    torch.cuda.synchronize()
    same_bits(host(rec), nb_ref, "receiver reconstruction")


# ---- batches of distinct tensors: every item == its single-tensor result ---------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 16])
@pytest.mark.parametrize("N,C", [(20, 24), (68, 136), (132, 144), (68, 528), (544, 576)])
def test_batches(N, C, B):
    from compactfusion_amd import _lib, codecs as K
    lib, ctx = _lib.load(), K.context(0)
    ins = [inputs(1000 * B + 17 * i + N + C, N, C) for i in range(B)]
    refs = [oracle(x, b) for x, b in ins]
    xs = [dev(x) for x, _ in ins]
    bs = [dev(b) for _, b in ins]
    nbs = [torch.empty_like(b) for b in bs]
    pks = [torch.zeros(K.packet_halves(CID, N, C, 0), dtype=torch.float16, device="cuda") for _ in range(B)]
    recs = [torch.empty_like(b) for b in bs]
    ic = _profile(ctx, lib, lambda: K.compress_batch(CID, xs, bs, nbs, pks, N, C, 0, update_cache=True))
    idd = _profile(ctx, lib, lambda: K.decompress_batch(CID, pks, bs, recs, N, C, 0))
    # the layer launch wants its statistics tiles co-resident (2 workgroups a CU, 8 slots kept free): 16 tensors of (544, 576) are
    # 2 x 17 x 16 = 544 tiles of 32 rows, more than the 504 of a 256-CU chip - the host check sends that batch to the multi-launch form
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    layer = C % 16 == 0 and ((C + 511) // 512) * ((N + 31) // 32) * B <= 2 * cus - 8
    assert ic == ([KID_LAYER] if layer else [KID_MM_COMPRESS, QUANT]) and idd == [DEQUANT], (ic, idd, layer)
    for i, (p_ref, n_ref) in enumerate(refs):
        same_packet(host(pks[i]), p_ref, ins[i][0], ins[i][1], f"packet item {i}/{B}")
        same_bits(host(nbs[i]), n_ref, f"sender state item {i}/{B}")
        same_bits(host(recs[i]), n_ref, f"reconstruction item {i}/{B}")
    assert lib.cfx_gate_errors(ctx) == 0


def test_gated_batch_of_16():
    """CFX_MAX_BATCH own tensors and as many looped-back peers in one layer launch"""
    N, C = 68, 144
    ins = [inputs(500 + i, N, C) for i in range(16)]
    assert _gated(N, C, ins, rounds=2, NP=16) == [KID_LAYER]


# ---- non-finite input: INT4's rules (NaN-propagating min / max, code 0) ----------------------------------------------------------------
@pytest.mark.parametrize("N,C", [(68, 136), (68, 144), (2052, 16)])
def test_nonfinite(N, C):
    from compactfusion_amd import codecs as K
    x, base = inputs(77 + N + C, N, C)
    rng = np.random.default_rng(N + C)
    for v in (np.nan, np.inf, -np.inf, np.nan):
        x[rng.integers(0, N, 3), rng.integers(0, C, 3)] = v
    x[0, 0] = base[0, 0] = np.inf                       # inf - inf
    x[N - 1, C - 1] = np.nan
    pkt_ref, nb_ref = oracle(x, base)
    xd, bd = dev(x), dev(base)
    for fused in (True, False):
        K.set_fused_finalize(fused)
        pkt, nb = K.compress(CID, xd, bd, N, C, 0, update_cache=True)
        rec = K.decompress(CID, pkt, bd, N, C, 0)
        torch.cuda.synchronize()
        same_bits(host(pkt), pkt_ref, f"packet (fused finalize {fused})")
        same_bits(host(nb), nb_ref, f"sender state (fused finalize {fused})")
        same_bits(host(rec), nb_ref, f"reconstruction (fused finalize {fused})")


# ---- a captured graph of plain compress + decompress, replayed (INT4's graph shapes, N a multiple of 4) -------------------------------
@pytest.mark.parametrize("N,C", [(36, 72), (68, 520)])
def test_graph_replay(N, C):
    from compactfusion_amd import codecs as K
    _, base = inputs(55 + N + C, N, C)
    state = dev(base)
    peer = dev(base)
    xin = torch.empty_like(state)
    pkt = torch.zeros(K.packet_halves(CID, N, C, 0), dtype=torch.float16, device="cuda")
    comp = K.prepare_compress(CID, [state], [state], [pkt], N, C, 0, update_cache=True)
    dec = K.prepare_decompress(CID, [pkt], [peer], [peer], N, C, 0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            comp([xin], side.cuda_stream)
            dec(side.cuda_stream)
    torch.cuda.synchronize()
    ostate = base.view(np.uint16).copy()
    for r in range(2):
        x, _ = inputs(900 + 31 * r + N, N, C)
        xin.copy_(dev(x))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        before = ostate
        p_ref, ostate = oracle(x, ostate.view(F16))
        same_packet(host(pkt), p_ref, x, before.view(F16), f"packet replay {r}")
        same_bits(host(state), ostate, f"sender state replay {r}")
        same_bits(host(peer), ostate, f"peer state replay {r}")


# ---- the stand-alone quantiser pair and the host state machine on the real kernels ----------------------------------------------------
def test_quantize_dequantize_pair():
    from compactfusion_amd.compact import compress_quantize as Q
    N, C = 64, 256
    torch.manual_seed(42)
    d = torch.randn(N, C).half()
    packed, scale, mn = Q.quantize_int2_minmax(d.cuda())
    want_pkt, want_recv = I.compress(host(d).reshape(N, C), None)
    qn = N * C // 8
    assert packed.shape == (N // 4, C) and np.array_equal(packed.cpu().numpy().reshape(-1), want_pkt[:qn].view(np.uint8))
    assert np.array_equal(host(scale).reshape(-1), want_pkt[qn:qn + C]) and np.array_equal(host(mn).reshape(-1), want_pkt[qn + C:])
    rec = Q.dequantize_int2_minmax(packed, scale, mn)
    same_bits(host(rec), R.bits(want_recv), "dequantize_int2_minmax")
    same_bits(host(rec), R.bits(R.sim_int2_minmax(host(d).reshape(N, C))), "the wire codec against the pinned simulation")
    same_bits(host(Q.sim_int2_minmax(d.cuda())), host(rec), "sim_int2_minmax (tensor arithmetic) against the kernels")


def _modes():
    from test_int2mm_host import MODES
    return MODES


@pytest.mark.parametrize("mode,kw,nwarm", _modes(), ids=[m[0] for m in _modes()])
def test_state_machine_on_the_kernels(mode, kw, nwarm, tmp_path):
    """compact_compress / compact_decompress with INT2_MINMAX: residual 1 with error feedback on and off, residual 0, residual 2 (the
    composition around the codec) against R.OracleCompact over the contract, bit for bit"""
    import compactfusion_amd.compact.main as cm
    from compactfusion_amd.collector import collector
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig
    from test_int2mm_host import _Oracle
    collector.init(collector.Collector(str(tmp_path), enabled=False))
    N, C = 64, 1024
    cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: None, **kw))
    orc_s = _Oracle(residual=kw["residual"], ef=kw["ef"], decay=kw.get("delta_decay_factor"))
    orc_r = _Oracle(residual=kw["residual"], ef=kw["ef"], decay=kw.get("delta_decay_factor"))
    skey, rkey = "0-0-k", "0-1-k"
    for t, x in enumerate(W.drift(11, (N, C), 5)):
        x4 = x.view(1, N, 8, C // 8)
        warm = t < nwarm
        typ, name = (T.WARMUP, "warmup") if warm else (T.INT2_MINMAX, "int2mm")
        pkt = cm.compact_compress(skey, x4.cuda(), typ, update_cache=True)
        want = orc_s.compress(skey, host(x4).reshape(1, N, 8, C // 8), name, True)
        same_bits(host(pkt).reshape(-1), want, f"{mode} step {t}: packet")
        rec = cm.compact_decompress(rkey, pkt.clone(), typ, x4.shape, update_cache=True)
        wrec = orc_r.decompress(rkey, want, name, x4.shape, True)
        same_bits(host(rec).reshape(-1), R.bits(wrec).reshape(-1), f"{mode} step {t}: reconstruction")
        if kw["residual"]:
            same_bits(host(cm.compact_cache().get_base(skey)).reshape(-1), R.bits(orc_s.base[skey]).reshape(-1), f"{mode} step {t}: sender state")
            same_bits(host(cm.compact_cache().get_base(rkey)).reshape(-1), R.bits(orc_r.base[rkey]).reshape(-1), f"{mode} step {t}: receiver state")
        if kw["residual"] == 2 and t >= 1:
            same_bits(host(cm.compact_cache().get_delta_base(skey)).reshape(-1), R.bits(orc_s.dbase[skey]).reshape(-1), f"{mode} step {t}: delta state")
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
            pkt, nb = I.residual_compress(x2, own, ef)
            peer = I.residual_decompress(pkt, peer, N, C)
        own = nb
        outs.append((R.bits(own).copy(), R.bits(peer).copy()))
    return outs


@pytest.mark.parametrize("ef", [True, False], ids=["ef", "noef"])
@pytest.mark.parametrize("api", ["ring", "gather"])
def test_plugin_call_one_layer_launch_per_layer(loop8, api, ef):
    """INT2_MINMAX through compact_fwd / compact_all_gather_kv with the lane off: ONE native op per layer, and that op is ONE codec launch
    (kernel id 31: k_minmax_layer<4, RW> with the peer-to-peer exchange inside) - no quantise (11), dequantise (12) or statistics (7, 8, 29)
    launch; every logical rank's state against the contract's replay bit for bit"""
    ring, cm, xlayer = loop8
    from compactfusion_amd import _lib, codecs as K
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig, PatchConfig
    lib, ctx = _lib.load(), K.context(0)
    L, STEPS = 2, 4
    shape, N, C = (1, 64, 16, 64), 64, 1024
    kw = dict(enabled=True, compress_func=lambda l, s: T.WARMUP if s == 0 else T.INT2_MINMAX, comp_rank=-1, residual=1, ef=ef, fastpath=False)
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
                assert got.count(KID_LAYER) == L and not any(got.count(k) for k in (QUANT, DEQUANT, KID_STATS, KID_FINALIZE, KID_MM_COMPRESS)), (api, s, got)
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


# ---- two rank processes on one GPU: compact_fwd end to end at world size 2 ----------------------------------------------------------
def _chain(xs):
    shape2 = (-1, xs[0].shape[-2] * xs[0].shape[-1])
    state = xs[0].numpy().reshape(shape2).copy()
    out = [R.bits(state).copy()]
    for x in xs[1:]:
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            _, state = I.residual_compress(x.numpy().reshape(state.shape), state)
        out.append(R.bits(state).copy())
    return out


@pytest.mark.parametrize("mode", ["ring", "gather"])
def test_two_processes_peer_to_peer(tmp_path, mode):
    """Two rank processes on one GPU, packets read in place through IPC mappings (validated across the ranks): every rank's view of every
    rank's K and V state, every step, == the contract's chain bit for bit.  STATES only: the worker body (tests/_dist_workers.py::w_xlayer,
    shared with the other codecs' tests) records no packets, so the packets are not compared here - a peer's state equals the chain only if
    the packet it decoded reconstructs as the contract's does; the packets themselves are held to the contract bit for bit by the
    single-process tests above."""
    from test_gpu_schedules import _spawn
    L, STEPS, shape = 3, 4, (1, 64, 8, 64)
    res = _spawn(W.w_xlayer, 2, tmp_path, "INT2_MINMAX", mode, -1, 1)
    for r in range(2):
        assert int(res[r]["n_ops"][0]) == 3 and int(res[r]["p2p"][0]) == 3 and int(res[r]["fell_back"][0]) == 0, "the peer-to-peer layer op was not taken"
    for l in range(L):
        want_k = [_chain(W.drift(17 + 10 * l + q, shape, STEPS)) for q in range(2)]
        want_v = [_chain(W.drift(27 + 10 * l + q, shape, STEPS)) for q in range(2)]
        for r in range(2):
            for s in range(STEPS):
                for q in range(2):
                    assert np.array_equal(res[r][f"g0/s{s}/l{l}/k{q}"].reshape(-1), want_k[q][s].reshape(-1)), (mode, l, r, s, q, "k")
                    assert np.array_equal(res[r][f"g0/s{s}/l{l}/v{q}"].reshape(-1), want_v[q][s].reshape(-1)), (mode, l, r, s, q, "v")


# ---- compact_fwd with the exchange lane ON (the default): the layer's chain on the CU-masked lane beside the attention blocks ----------
from test_gpu_lane import W as LW, _late, loopback      # noqa: E402,F401  (the 8-logical-rank ring over the loop-back collective)


@pytest.mark.parametrize("ef", [True, False], ids=["ef", "noef"])
def test_lane_ring_forward(loopback, monkeypatch, ef):
    """tests/test_gpu_lane.py::test_lane_ring_forward_vs_oracle at its default settings ("auto": compact_fwd forks to the lane and joins back)
    with INT2_MINMAX: the owner's and every peer's state against the contract's replay bit for bit, the merged attention output against
    one attention over what the rank holds, the lane plan engaged, no gate error"""
    ring, cm = loopback
    from compactfusion_amd import _lib, codecs as K
    from compactfusion_amd.compact import COMPACT_COMPRESS_TYPE as T, CompactConfig
    from compactfusion_amd.compact.attention import block_attention
    monkeypatch.delenv("CFX_RING_EXCHANGE_STREAM", raising=False)
    monkeypatch.setenv("CFX_LANE", "auto")
    L, STEPS = 3, 5
    shape, N, C = (1, 64, 8, 64), 64, 512
    cm.compact_init(CompactConfig(enabled=True, compress_func=lambda l, s: T.WARMUP if s == 0 else T.INT2_MINMAX, comp_rank=-1,
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
            outs = {}
            for l in range(L):
                out, lse, _ = ring.compact_fwd(dq[l][s], _late(dk[l][s]), _late(dv[l][s]), causal=False, mod_idx=l, current_iter=s)
                assert torch.cuda.current_stream(dev0).cuda_stream == stream.cuda_stream, "the caller's stream is the current stream again"
                outs[l] = (out * 1.0, lse)
            torch.cuda.synchronize()
            cache = cm.compact_cache()
            for l in range(L):
                for n in ("k", "v"):
                    for r in range(LW):
                        w = want[(l, n)][s][0 if (r == 0 or ef) else 1]
                        assert np.array_equal(host(cache.get_base(f"{l}-{r}-{n}")).reshape(N, C), w.reshape(N, C)), (s, l, n, r)
                kk = [dk[l][s]] + [cache.get_base(f"{l}-{(0 - t) % LW}-k").view(shape) for t in range(1, LW)]
                vv = [dv[l][s]] + [cache.get_base(f"{l}-{(0 - t) % LW}-v").view(shape) for t in range(1, LW)]
                ref_o, ref_l = block_attention(dq[l][s], torch.cat(kk, dim=1), torch.cat(vv, dim=1), 0.0, None, causal=False)
                torch.testing.assert_close(outs[l][0].float(), ref_o.float(), rtol=2e-3, atol=2e-3)
                torch.testing.assert_close(outs[l][1].float(), ref_l.float(), rtol=1e-3, atol=1e-3)
    exs = [e for e in ring._xbuf.values() if e.sig is not None]
    assert exs and all(e.lane for e in exs), "the native per-layer lane plan was not used"
    assert len(ring._steady) == L, "the steady-state lane never engaged"
    assert _lib.load().cfx_gate_errors(K.context(0)) == 0
