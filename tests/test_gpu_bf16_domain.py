"""The bf16 instantiations of the 1-bit and 2-bit codecs (CFX_ELEM_BF16) through every form tests/test_gpu_codec_domain.py drives the
fp16 ones through, and over the bf16 value domain of tests/_bf16_cases.py (GPU box only, -m gpu).

Reference: tests/bf16_contract.py, bit for bit - packets, sender states, receiver reconstructions, looped-back peer states - and the
definition checked independently (tests/_bf16_f64_check.py) on what the GPU returned.  Forms: (b) in-launch finalize off and on with
every rows-per-tile override, explicit statistics tile heights, (c) batches of 1 / 3 / CFX_MAX_BATCH, (d) the gated layer call with
error feedback and looped-back peers over rounds, and with the one-launch forms switched off, (e) a captured graph replayed, (f) the
ride-along reconstruction group of cfx_compress_batch_ex, (g) a stream masked below 128 CUs, (h) the value cases through the plain
call, finalize off and the layer call, and hand-built tie packets through cfx_decompress_batch and cfx_int2_quantize.  The last test
proves the coverage: which bf16 kernels ran, and that each codec's layer call took the one-launch form and the fallback."""
import ctypes

import numpy as np
import pytest
import torch

import _bf16_cases as V
import _bf16_f64_check as BF
import _domain_cases as D
import bf16_contract as BC

pytestmark = pytest.mark.gpu

NAME = {1: "binary", 2: "int2"}
BFLAG = BC.ELEM_BF16
KID_LAYER = 31
UPD = 1
bits = BC.torch_bits


def dev(u16):
    return torch.from_numpy(np.ascontiguousarray(u16).view(np.int16).copy()).view(torch.bfloat16).cuda()


def same_bits(a, b, what):
    a = np.asarray(a).view(np.uint16).reshape(-1)
    b = np.asarray(b).view(np.uint16).reshape(-1)
    assert a.size == b.size, f"{what}: {a.size} words against {b.size}"
    bad = a != b
    assert not bad.any(), f"{what}: {int(bad.sum())}/{a.size} differ (first at {int(np.argmax(bad))})"


def inputs(seed, N, C):
    rng = np.random.default_rng(seed)
    base = V.bf16_bits(0.5 * rng.standard_normal((N, C)))
    x = V.bf16_bits(V.bf16_f32(base) + 0.2 * rng.standard_normal((N, C)).astype(np.float32))
    return x, base


def _lib_ctx():
    from compactfusion_amd import _lib, codecs as K
    return _lib, _lib.load(), K.context(0)


@pytest.fixture(autouse=True)
def _defaults():
    from compactfusion_amd import codecs as K
    _, lib, ctx = _lib_ctx()
    yield
    torch.cuda.synchronize()
    K.set_fused_finalize(True)
    K.set_rows_per_tile(0)
    lib.cfx_set_stats_rows(ctx, 0)
    lib.cfx_set_gated_launch(ctx, 1)
    assert lib.cfx_gate_errors(ctx) == 0


def _profile(fn):
    """kernel ids of what fn launched (every call in fn is this module's own, made with CFX_ELEM_BF16)"""
    _, lib, ctx = _lib_ctx()
    torch.cuda.synchronize()
    assert lib.cfx_profile_enable(ctx, 64, 0xffffffff, 1) == 0
    try:
        fn()
        torch.cuda.synchronize()
        ids, ms = (ctypes.c_int * 64)(), (ctypes.c_float * 64)()
        n = lib.cfx_profile_read(ctx, ids, ms, 64)
    finally:
        lib.cfx_profile_enable(ctx, 0, 0, 1)
    return [ids[i] for i in range(n)]


def _cases(pool, extra=()):
    return [pytest.param(cid, N, C, id=f"{NAME[cid]}-{N}x{C}") for cid in (1, 2) for N, C in list(pool) + list(extra) if D.legal(NAME[cid], N, C)]


def plain(cid, xd, bd, N, C, rec=True):
    """K.compress (+ K.decompress) with bf16 tensors: (packet bits, state bits, reconstruction bits)"""
    from compactfusion_amd import codecs as K
    pkt, nb = K.compress(cid, xd, bd, N, C, 0, update_cache=True)
    r = K.decompress(cid, pkt, bd, N, C, 0, recon=torch.empty(N, C, dtype=torch.bfloat16, device="cuda")) if rec else None
    torch.cuda.synchronize()
    assert nb.dtype == torch.bfloat16
    return bits(pkt), bits(nb).reshape(N, C), None if r is None else bits(r).reshape(N, C)


# ---- (b) the multi-launch forms, every rows-per-tile override, explicit statistics tile heights -------------------------------------
@pytest.mark.parametrize("cid,N,C", _cases(D.FINALIZE_OFF))
def test_finalize_off_row_tiles_and_stats_rows(cid, N, C):
    from compactfusion_amd import codecs as K
    _, lib, ctx = _lib_ctx()
    name = NAME[cid]
    x, base = inputs(N * 7 + C, N, C)
    pkt_ref, nb_ref = BC.compress(name, x, base)
    xd, bd = dev(x), dev(base)
    K.set_fused_finalize(False)
    for rows in (0,) + D.ROWS_PER_TILE:
        K.set_rows_per_tile(rows)
        p, nb, rec = plain(cid, xd, bd, N, C)
        same_bits(p, pkt_ref, f"packet (finalize off, rows {rows})")
        same_bits(nb, nb_ref, f"sender state (finalize off, rows {rows})")
        same_bits(rec, nb_ref, f"reconstruction (finalize off, rows {rows})")
        if rows == 0:
            BF.check(name, x, base, p, nb)
    K.set_fused_finalize(True)
    for rows in D.ROWS_PER_TILE:
        K.set_rows_per_tile(rows)
        p, nb, rec = plain(cid, xd, bd, N, C)
        same_bits(p, pkt_ref, f"packet (rows {rows})")
        same_bits(nb, nb_ref, f"sender state (rows {rows})")
        same_bits(rec, nb_ref, f"reconstruction (rows {rows})")
    K.set_rows_per_tile(0)
    for rows in (16, 64, 128):
        assert lib.cfx_set_stats_rows(ctx, rows) == 0
        p, nb, _ = plain(cid, xd, bd, N, C, rec=False)
        same_bits(p, pkt_ref, f"packet (statistics rows {rows})")
        same_bits(nb, nb_ref, f"sender state (statistics rows {rows})")
    # base None under finalize off: the state is bf16(recv)
    if N * C <= 1 << 20:
        lib.cfx_set_stats_rows(ctx, 0)
        K.set_fused_finalize(False)
        p0_ref, nb0_ref = BC.compress(name, x, None)
        p, nb, rec = plain(cid, xd, None, N, C)
        same_bits(p, p0_ref, "packet (base None, finalize off)")
        same_bits(nb, nb0_ref, "state (base None, finalize off)")
        same_bits(rec, nb0_ref, "reconstruction (base None, finalize off)")


# ---- (c) batches of distinct tensors --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, D.MAX_BATCH])
@pytest.mark.parametrize("cid,N,C", _cases(D.BATCH_SHAPES))
def test_batches(cid, N, C, B):
    from compactfusion_amd import codecs as K
    name = NAME[cid]
    ins = [inputs(1000 * B + 17 * i + N + C, N, C) for i in range(B)]
    refs = [BC.compress(name, x, b) for x, b in ins]
    xs = [dev(x) for x, _ in ins]
    bs = [dev(b) for _, b in ins]
    nbs = [torch.empty_like(b) for b in bs]
    pks = [torch.zeros(K.packet_halves(cid, N, C), dtype=torch.float16, device="cuda") for _ in range(B)]
    recs = [torch.empty_like(b) for b in bs]
    K.compress_batch(cid, xs, bs, nbs, pks, N, C, 0, update_cache=True)
    K.decompress_batch(cid, pks, bs, recs, N, C, 0)
    torch.cuda.synchronize()
    for i, (p_ref, n_ref) in enumerate(refs):
        same_bits(bits(pks[i]), p_ref, f"packet item {i}/{B}")
        same_bits(bits(nbs[i]), n_ref, f"sender state item {i}/{B}")
        same_bits(bits(recs[i]), n_ref, f"reconstruction item {i}/{B}")
        same_bits(bits(bs[i]), ins[i][1], f"base item {i}/{B} was written")
    BF.check(name, ins[B - 1][0], ins[B - 1][1], bits(pks[B - 1]), bits(nbs[B - 1]).reshape(N, C))


# ---- (d) the gated layer call ---------------------------------------------------------------------------------------------------------
class Gated:
    """cfx_compress_batch_gated with CFX_ELEM_BF16: B own tensors (error feedback in place), NP looped-back peer states"""

    def __init__(self, cid, N, C, pairs, NP=3):
        from compactfusion_amd import codecs as K
        self._lib, self.lib, self.ctx = _lib_ctx()
        self.cid, self.N, self.C, self.B, self.NP = cid, N, C, len(pairs), NP
        B = self.B
        self.xd = [dev(x) for x, _ in pairs]
        self.own = [dev(b) for _, b in pairs]
        self.src = [g % B for g in range(NP)]
        self.peer = [dev(pairs[s][1]) for s in self.src]
        self.pk = [torch.zeros(K.packet_halves(cid, N, C), dtype=torch.float16, device="cuda") for _ in range(B)]
        self.wsb = self.lib.cfx_workspace_bytes(cid | BFLAG, N, C, 0, B)
        self.ws = torch.empty(max(self.wsb, 16), dtype=torch.uint8, device="cuda")
        L = self._lib
        self.comp = (L.CompItem * B)(*[L.CompItem(self.xd[i].data_ptr(), self.own[i].data_ptr(), self.own[i].data_ptr(), self.pk[i].data_ptr())
                                       for i in range(B)])
        self.gated = (L.DecompItem * NP)(*[L.DecompItem(self.pk[self.src[g]].data_ptr(), self.peer[g].data_ptr(), self.peer[g].data_ptr())
                                           for g in range(NP)])
        self.state = [np.array(b, copy=True) for _, b in pairs]
        self.xs = [x for x, _ in pairs]
        torch.cuda.synchronize()

    def call(self, stream=None):
        sh = torch.cuda.current_stream().cuda_stream if stream is None else stream
        rc = self.lib.cfx_compress_batch_gated(self.ctx, self.cid | BFLAG, self.N, self.C, 0, UPD, self.B, self.comp, 0, None, self.NP, self.gated,
                                               self.ws.data_ptr(), self.wsb, sh)
        assert rc == 0, self.lib.cfx_last_error_string(self.ctx)

    def check(self, what, definition=False):
        """advance the contract by one step of the same activations and compare"""
        torch.cuda.synchronize()
        assert self.lib.cfx_gate_errors(self.ctx) == 0, what
        name = NAME[self.cid]
        for i in range(self.B):
            before = self.state[i]
            p, self.state[i] = BC.compress(name, self.xs[i], before)
            same_bits(bits(self.pk[i]), p, f"{what}: packet {i}")
            same_bits(bits(self.own[i]), self.state[i], f"{what}: own state {i}")
            if definition and i == 0:
                BF.check(name, self.xs[i], before, bits(self.pk[i]), bits(self.own[i]).reshape(self.N, self.C))
        for g in range(self.NP):
            same_bits(bits(self.peer[g]), self.state[self.src[g]], f"{what}: peer state {g}")


@pytest.mark.parametrize("cid,N,C", _cases(D.GATED_SHAPES))
def test_gated_layer(cid, N, C):
    g = Gated(cid, N, C, [inputs(7 * N + C + i, N, C) for i in range(2)])
    for t in range(2 if N * C > 4 << 20 else 3):
        g.call()
        g.check(f"round {t}", definition=t == 0)


@pytest.mark.parametrize("cid", [1, 2])
def test_gated_layer_with_the_one_launch_forms_off(cid):
    """cfx_set_gated_launch(ctx, 0): compress ; reconstruct in stream order at a shape that otherwise takes the one-launch form"""
    N, C = V.LAYER
    g = Gated(cid, N, C, [inputs(91 + i, N, C) for i in range(2)], NP=6)
    assert g.lib.cfx_set_gated_launch(g.ctx, 0) == 0
    ids = _profile(g.call)
    assert KID_LAYER not in ids and len(ids) >= 3, ids
    g.check("gated launch off, round 0")
    g.call()
    g.check("gated launch off, round 1")
    assert g.lib.cfx_set_gated_launch(g.ctx, 1) == 0
    ids = _profile(g.call)
    assert ids == [KID_LAYER], ids
    g.check("gated launch on again")


# ---- (e) a captured graph of plain compress + decompress, replayed ---------------------------------------------------------------------
@pytest.mark.parametrize("cid,N,C", _cases(D.GRAPH_SHAPES))
def test_graph_replay(cid, N, C):
    from compactfusion_amd import codecs as K
    name = NAME[cid]
    _, base = inputs(55 + N + C, N, C)
    state, peer = dev(base), dev(base)
    xin = torch.empty_like(state)
    pkt = torch.zeros(K.packet_halves(cid, N, C), dtype=torch.float16, device="cuda")
    comp = K.prepare_compress(cid, [state], [state], [pkt], N, C, 0, update_cache=True)
    dec = K.prepare_decompress(cid, [pkt], [peer], [peer], N, C, 0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            comp([xin], side.cuda_stream)
            dec(side.cuda_stream)
    torch.cuda.synchronize()
    same_bits(bits(state), base, "capture must not execute")
    ostate = base.copy()
    for r in range(2):
        x, _ = inputs(900 + 31 * r + N, N, C)
        xin.copy_(dev(x))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        p_ref, ostate = BC.compress(name, x, ostate)
        same_bits(bits(pkt), p_ref, f"packet replay {r}")
        same_bits(bits(state), ostate, f"sender state replay {r}")
        same_bits(bits(peer), ostate, f"peer state replay {r}")


# ---- (f) the ride-along reconstruction group of cfx_compress_batch_ex (1-bit) ---------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["finalize-on", "finalize-off"])
@pytest.mark.parametrize("N,C", [(129, 144), (130, 1024), (544, 3072), (2, 23560)])
def test_ride_along_items(N, C, fused):
    """two compress items and three ride items (an older packet onto states of their own): inside k_absmean_compress with the in-launch
    finalize, a k_binary_dequant launch of their own without (and at CB = 47, which has no in-launch finalize either way)"""
    from compactfusion_amd import codecs as K
    L, lib, ctx = _lib_ctx()
    K.set_fused_finalize(fused)
    B, NR = 2, 3
    ins = [inputs(300 + i + N, N, C) for i in range(B)]
    old_x, old_b = inputs(77 + C, N, C)
    old_pkt, _ = BC.compress("binary", old_x, old_b)
    ride_base = [inputs(400 + i + N, N, C)[1] for i in range(NR)]
    xd, bd = [dev(x) for x, _ in ins], [dev(b) for _, b in ins]
    nbd = [torch.empty_like(b) for b in bd]
    pk = [torch.zeros(K.packet_halves(1, N, C), dtype=torch.float16, device="cuda") for _ in range(B)]
    opk = torch.from_numpy(old_pkt.view(np.int16).copy()).view(torch.float16).cuda()
    rb = [dev(b) for b in ride_base]
    rr = [rb[0], torch.empty_like(rb[1]), rb[2]]                  # recon aliasing base, and a tensor of its own
    comp = (L.CompItem * B)(*[L.CompItem(xd[i].data_ptr(), bd[i].data_ptr(), nbd[i].data_ptr(), pk[i].data_ptr()) for i in range(B)])
    ride = (L.DecompItem * NR)(*[L.DecompItem(opk.data_ptr(), rb[i].data_ptr(), rr[i].data_ptr()) for i in range(NR)])
    wsb = lib.cfx_workspace_bytes(1 | BFLAG, N, C, 0, B)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
    sh = torch.cuda.current_stream().cuda_stream
    ids = _profile(lambda: lib.cfx_compress_batch_ex(ctx, 1 | BFLAG, N, C, 0, UPD, B, comp, NR, ride, ws.data_ptr(), wsb, sh))
    in_launch = fused and (C + 511) // 512 <= D.TICK_MAX_CB
    assert ids == ([27, 16] if in_launch else [1, 3, 4, 16]), ids
    for i in range(B):
        p, nb = BC.compress("binary", *ins[i])
        same_bits(bits(pk[i]), p, f"packet {i}")
        same_bits(bits(nbd[i]), nb, f"sender state {i}")
    for i in range(NR):
        want = BC.decompress("binary", old_pkt, ride_base[i], N, C)
        same_bits(bits(rr[i]), want, f"ride item {i}")
        BF.check_state("binary", ride_base[i], old_pkt, bits(rr[i]).reshape(N, C))


# ---- (g) a stream masked below 128 CUs --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,N,C", _cases([(129, 144), (130, 1024), (544, 3072)]))
def test_masked_stream(cid, N, C):
    """plain in-order launches on the exchange lane's stream (fewer than 128 CUs): compress, decompress (1-bit: k_binary_dequant<4>), and
    the gated call, which a stream of fewer than 128 CUs sends down the multi-launch form (cfx_i_absmean_compress)"""
    from compactfusion_amd import codecs as K, lanes
    L, lib, ctx = _lib_ctx()
    name = NAME[cid]
    ex = lanes.exchange_stream(0)
    assert lanes.lane(0).exchange_cus < 128
    x, base = inputs(5 * N + C, N, C)
    p_ref, nb_ref = BC.compress(name, x, base)
    xd, bd = dev(x), dev(base)
    nb, rec = torch.empty_like(bd), torch.empty_like(bd)
    pkt = torch.zeros(K.packet_halves(cid, N, C), dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()

    def run():
        K.compress_batch(cid, [xd], [bd], [nb], [pkt], N, C, 0, update_cache=True, stream=ex)
        K.decompress_batch(cid, [pkt], [bd], [rec], N, C, 0, stream=ex)
    ids = _profile(run)
    assert ids == ([27, 16, 4] if cid == 1 else [28, 5, 6]), ids
    same_bits(bits(pkt), p_ref, "packet (masked stream)")
    same_bits(bits(nb), nb_ref, "sender state (masked stream)")
    same_bits(bits(rec), nb_ref, "reconstruction (masked stream)")
    BF.check_state(name, base, bits(pkt), bits(rec).reshape(N, C))
    g = Gated(cid, N, C, [inputs(13 * N + C + i, N, C) for i in range(2)], NP=6)
    ids = _profile(lambda: g.call(ex.cuda_stream))
    assert ids == ([27, 16, 4] if cid == 1 else [28, 5, 6]), f"the layer call on a masked stream runs the multi-launch form, got {ids}"
    g.check("gated call on the masked stream, round 0")
    g.call(ex.cuda_stream)
    g.check("gated call on the masked stream, round 1")


# ---- (h) the value domain ----------------------------------------------------------------------------------------------------------------
VALUE = [pytest.param(cid, case, N, C, id=f"{NAME[cid]}-{case}-{N}x{C}") for cid in (1, 2) for case, N, C in V.all_cases()]


@pytest.mark.parametrize("cid,case,N,C", VALUE)
def test_value_cases(cid, case, N, C):
    """every value case through the plain call, the plain call with the in-launch finalize off, and the gated layer call (own state in
    place, looped-back peers); the drift cases launch the layer call twice in a row (the second meets the first one's tags)"""
    from compactfusion_amd import codecs as K
    name = NAME[cid]
    x, base = V.build(case, N, C)
    p_ref, nb_ref = BC.compress(name, x, base)
    xd, bd = dev(x), None if base is None else dev(base)
    for fused in (True, False):
        K.set_fused_finalize(fused)
        p, nb, rec = plain(cid, xd, bd, N, C)
        same_bits(p, p_ref, f"packet (finalize {fused})")
        same_bits(nb, nb_ref, f"sender state (finalize {fused})")
        same_bits(rec, nb_ref, f"reconstruction (finalize {fused})")
        if fused:
            BF.check(name, x, base, p, nb)
    K.set_fused_finalize(True)
    if base is None:
        return                                        # (the layer call updates a state in place: it has one)
    pairs = [(x, base), V.build(case, N, C, rep=1)]
    g = Gated(cid, N, C, pairs, NP=4)
    g.call()
    if case in V.DRIFTS:
        g.check("layer call")
        g.xs = [V.build(case, N, C, rep=2 + i)[0] for i in range(2)]
        for i in range(2):
            g.xd[i].copy_(dev(g.xs[i]))
        torch.cuda.synchronize()
        g.call()
        g.check("second layer call, the arena holds the first one's tags")
    else:
        g.check("layer call", definition=True)


@pytest.mark.parametrize("N,C", V.TIE_SHAPES)
@pytest.mark.parametrize("cid", [1, 2])
def test_round_to_even_ties_in_the_state(cid, N, C):
    """hand-built packets through cfx_decompress_batch: fp32(base) + fp32(recv) exactly halfway between two bf16 values, lower neighbour
    even and odd (tests/test_bf16_domain_f64.py counts them), zero scales with both sign bits; with and without a base, recon in place
    and apart; on the full stream and on the masked one.  2-bit: the same ties through cfx_int2_quantize, scales planted in the packet."""
    from compactfusion_amd import codecs as K, lanes
    L, lib, ctx = _lib_ctx()
    name = NAME[cid]
    base, pkt = V.tie_packet(name, N, C)
    want, want0 = BC.decompress(name, pkt, base, N, C), BC.decompress(name, pkt, None, N, C)
    pk = torch.from_numpy(pkt.view(np.int16).copy()).view(torch.float16).cuda()
    bd = dev(base)
    for stream in (None, lanes.exchange_stream(0)):
        rec, rec0, inpl = torch.empty_like(bd), torch.empty_like(bd), dev(base)
        torch.cuda.synchronize()
        K.decompress_batch(cid, [pk, pk, pk], [bd, None, inpl], [rec, rec0, inpl], N, C, 0, stream=stream)
        torch.cuda.synchronize()
        same_bits(bits(rec), want, "reconstruction of the tie packet")
        same_bits(bits(inpl), want, "reconstruction of the tie packet, in place")
        same_bits(bits(rec0), want0, "reconstruction of the tie packet, base None")
        BF.check_state(name, base, pkt, bits(rec).reshape(N, C))
        BF.check_state(name, None, pkt, bits(rec0).reshape(N, C))
    if cid == 2:
        x, b, tok, chan = V.tie_quantize(N, C)
        p_ref, nb_ref = BC.int2_quantize(x, b, tok, chan)
        pq = torch.from_numpy(np.asarray(p_ref).view(np.int16).copy()).view(torch.float16).cuda()
        pq.view(torch.uint8)[:N * C // 4] = 0
        xd, bq, nb = dev(x), dev(b), torch.zeros(N, C, dtype=torch.bfloat16, device="cuda")
        items = (L.CompItem * 1)(L.CompItem(xd.data_ptr(), bq.data_ptr(), nb.data_ptr(), pq.data_ptr()))
        assert lib.cfx_int2_quantize(ctx, N, C, UPD | L.FLAG_ELEM_BF16, 1, items, None) == 0, lib.cfx_last_error_string(ctx)
        torch.cuda.synchronize()
        same_bits(bits(pq), p_ref, "cfx_int2_quantize packet")
        same_bits(bits(nb), nb_ref, "cfx_int2_quantize state")
        BF.check_state("int2", b, p_ref, bits(nb).reshape(N, C))


# ---- coverage: which bf16 kernels ran -------------------------------------------------------------------------------------------------
def test_coverage_of_the_bf16_launches():
    """Shapes from the dispatch rules of csrc/cfx_absmean.hip and cfx_api.hip, not by trial.  gated_one_launch: C % 128 == 0, CB <= 46, a
    32-row statistics tile (cfx_i_fused_rows: CB * ceil(N / 64) * batch < 768), a stream of >= 128 CUs; 2-bit: CB * P * batch tiles
    co-resident.  (17, 1920): CB 4, P 1, 8 tiles; (544, 3072): CB 6, P 17, 204 tiles -> id 31 alone.  (544, 576), (129, 144): C % 128
    != 0 -> the fallback: 27 / 28 (statistics + in-launch finalize), 16 (1-bit error feedback) / 5 (2-bit quantise), 4 / 6 (peers).
    Finalize off: 1 / 2 (statistics), 3 (finalize).  The profile log does not tell element types apart: every call recorded here is made
    by this test with CFX_ELEM_BF16."""
    from compactfusion_amd import codecs as K
    seen = {1: set(), 2: set()}
    forms = {1: {}, 2: {}}
    for cid in (1, 2):
        for N, C in ((17, 1920), (544, 3072), (544, 576), (129, 144)):
            g = Gated(cid, N, C, [inputs(i, N, C) for i in range(2)])
            ids = _profile(g.call)
            seen[cid].update(ids)
            forms[cid][(N, C)] = ids
        for N, C in ((17, 1920), (544, 3072)):
            assert forms[cid][(N, C)] == [KID_LAYER], (cid, N, C, forms[cid][(N, C)])
        for N, C in ((544, 576), (129, 144)):
            assert forms[cid][(N, C)] == ([27, 16, 4] if cid == 1 else [28, 5, 6]), (cid, N, C, forms[cid][(N, C)])
        N, C = 129, 144
        x, base = inputs(3, N, C)
        xd, bd = dev(x), dev(base)
        K.set_fused_finalize(False)
        ids = _profile(lambda: plain(cid, xd, bd, N, C))
        assert ids == ([1, 3, 16, 4] if cid == 1 else [2, 3, 5, 6]), ids
        seen[cid].update(ids)
        K.set_fused_finalize(True)
    assert seen[1] == {1, 3, 4, 16, 27, 31}, seen[1]
    assert seen[2] == {2, 3, 5, 6, 28, 31}, seen[2]
    assert seen[1] | seen[2] == {1, 2, 3, 4, 5, 6, 16, 27, 28, 31}
