"""The codecs over the whole shape and value domain the C-ABI accepts (GPU box only, -m gpu).

Shapes: tests/_domain_cases.py (odd N, C % 16 == 8, partial column blocks, CB = 46 / 47, unaligned packet tails, model shards).  Every
codec and legal shape, bit for bit against the oracle (the C oracle above 4M elements) and against the float64 definition
(tests/_f64_check.py), through: (a) the plain calls, (b) the multi-launch forms (in-launch finalize off, rows per tile 16 .. 128),
(c) batches of 1 / 3 / CFX_MAX_BATCH, (d) the gated layer call with error feedback and looped-back peers over rounds, (e) a captured
graph replayed.  The test proves its own coverage: the layer form and the fallback form of every codec that has both ran.
Non-finite input: golden G16 (tests/_nonfinite.py) through the plain, the multi-launch and the layer forms."""
import numpy as np
import pytest
import torch

import _domain_cases as D
import _f64_check as F
import _nonfinite as NF
from _gpu_codec import BIG, KID_LAYER, _gated_layer, _profile, dev, host, inputs, oracle, same_bits, same_packet

pytestmark = pytest.mark.gpu

F16 = np.float16


def _cases(pool=None):
    out = []
    for (name, cid, param), tag in zip(D.CODECS, D.CODEC_IDS):
        shapes = D.shapes_for(name, param) if pool is None else D.subset(name, param, pool)
        out += [pytest.param(name, cid, param, N, C, id=f"{tag}-{N}x{C}") for N, C in shapes]
    return out


@pytest.fixture(autouse=True)
def _defaults():
    from compactfusion_amd import codecs as K
    yield
    K.set_fused_finalize(True)
    K.set_rows_per_tile(0)


# ---- (a) the plain calls ----
@pytest.mark.parametrize("name,cid,param,N,C", _cases())
def test_plain(name, cid, param, N, C):
    from compactfusion_amd import codecs as K
    x, base = inputs(N * 131 + C, N, C)
    pkt_ref, nb_ref = oracle(name, x, base, param, N, C)
    xd, bd = dev(x), dev(base)
    pkt, nb = K.compress(cid, xd, bd, N, C, param, update_cache=True)
    torch.cuda.synchronize()
    hp, hn = host(pkt), host(nb).reshape(N, C)
    same_packet(name, hp, pkt_ref, x, base, "packet")
    same_bits(hn, nb_ref, "sender state")
    F.check(name, param, x, base, hp, hn)
    rec = K.decompress(cid, pkt, bd, N, C, param)
    torch.cuda.synchronize()
    same_bits(host(rec), nb_ref, "receiver reconstruction")
    pkt2, nb2 = K.compress(cid, xd, bd, N, C, param, update_cache=False)
    torch.cuda.synchronize()
    assert nb2 is None
    same_packet(name, host(pkt2), pkt_ref, x, base, "packet (update_cache off)")
    pkt3, nb3 = K.compress(cid, xd, bd, N, C, param, update_cache=True, ef=False)
    torch.cuda.synchronize()
    same_packet(name, host(pkt3), pkt_ref, x, base, "packet (ef off)")
    same_bits(host(nb3), x.view(np.uint16), "state (ef off) == x")
    # base=None: the codec on x itself
    p0_ref, r0_ref = oracle(name, x, None, param, N, C)
    p0, r0 = K.compress(cid, xd, None, N, C, param, update_cache=True)
    rec0 = K.decompress(cid, p0, None, N, C, param)
    torch.cuda.synchronize()
    same_packet(name, host(p0), p0_ref, x, None, "packet (base None)")
    same_bits(host(r0), r0_ref, "state (base None)")
    same_bits(host(rec0), r0_ref, "reconstruction (base None)")


# ---- (b) the multi-launch forms: in-launch finalize off, every rows-per-tile override ----
@pytest.mark.parametrize("name,cid,param,N,C", _cases(D.FINALIZE_OFF))
def test_finalize_off_and_row_tiles(name, cid, param, N, C):
    from compactfusion_amd import codecs as K
    x, base = inputs(N * 7 + C, N, C)
    pkt_ref, nb_ref = oracle(name, x, base, param, N, C)
    xd, bd = dev(x), dev(base)
    K.set_fused_finalize(False)
    for rows in (0,) + D.ROWS_PER_TILE:
        K.set_rows_per_tile(rows)
        pkt, nb = K.compress(cid, xd, bd, N, C, param, update_cache=True)
        rec = K.decompress(cid, pkt, bd, N, C, param)
        torch.cuda.synchronize()
        same_packet(name, host(pkt), pkt_ref, x, base, f"packet (finalize off, rows {rows})")
        same_bits(host(nb), nb_ref, f"sender state (finalize off, rows {rows})")
        same_bits(host(rec), nb_ref, f"reconstruction (finalize off, rows {rows})")
    K.set_fused_finalize(True)
    for rows in D.ROWS_PER_TILE:
        K.set_rows_per_tile(rows)
        pkt, nb = K.compress(cid, xd, bd, N, C, param, update_cache=True)
        torch.cuda.synchronize()
        same_packet(name, host(pkt), pkt_ref, x, base, f"packet (rows {rows})")
        same_bits(host(nb), nb_ref, f"sender state (rows {rows})")


# ---- (c) batches of distinct tensors: every item == its single-tensor result ----
@pytest.mark.parametrize("B", [1, 3, D.MAX_BATCH])
@pytest.mark.parametrize("name,cid,param,N,C", _cases(D.BATCH_SHAPES))
def test_batches(name, cid, param, N, C, B):
    from compactfusion_amd import codecs as K
    ins = [inputs(1000 * B + 17 * i + N + C, N, C) for i in range(B)]
    refs = [oracle(name, x, b, param, N, C) for x, b in ins]
    xs = [dev(x) for x, _ in ins]
    bs = [dev(b) for _, b in ins]
    nbs = [torch.empty_like(b) for b in bs]
    pks = [torch.zeros(K.packet_halves(cid, N, C, param), dtype=torch.float16, device="cuda") for _ in range(B)]
    recs = [torch.empty_like(b) for b in bs]
    K.compress_batch(cid, xs, bs, nbs, pks, N, C, param, update_cache=True)
    K.decompress_batch(cid, pks, bs, recs, N, C, param)
    torch.cuda.synchronize()
    for i, (p_ref, n_ref) in enumerate(refs):
        same_packet(name, host(pks[i]), p_ref, ins[i][0], ins[i][1], f"packet item {i}/{B}")
        same_bits(host(nbs[i]), n_ref, f"sender state item {i}/{B}")
        same_bits(host(recs[i]), n_ref, f"reconstruction item {i}/{B}")


# ---- (d) the gated layer call: own error feedback + looped-back peers, over rounds (_gpu_codec._gated_layer) ----
def _form(ids):
    return "layer" if ids == [KID_LAYER] else "fallback"


@pytest.mark.parametrize("name,cid,param,N,C", _cases(D.GATED_SHAPES))
def test_gated_layer(name, cid, param, N, C):
    rounds = 2 if N * C > BIG else 3
    _gated_layer(name, cid, param, N, C, B=2, NP=3, rounds=rounds, seed=7 * N + C)


@pytest.mark.parametrize("name,cid", [("int4", 3), ("int8", 4)])
def test_minmax_tile_count_crossing(name, cid):
    """(2049, 23552): 46 column blocks x 33 row tiles = 1518 layer tiles for one tensor, 3036 for a batch of 2 - across MML_MAX_TILES
    (2048).  Plain batch calls of 1 and 2 tensors: bit for bit, whichever form each takes."""
    from compactfusion_amd import _lib, codecs as K
    lib = _lib.load()
    ctx = K.context(0)
    N, C, B2 = D.TILE_CROSSING
    if name == "int4" and N % 2:
        N += 1
    ins = [inputs(4242 + i, N, C) for i in range(B2)]
    refs = [oracle(name, x, b, 0, N, C) for x, b in ins]
    forms = set()
    for B in (1, B2):
        xs = [dev(x) for x, _ in ins[:B]]
        bs = [dev(b) for _, b in ins[:B]]
        pks = [torch.zeros(K.packet_halves(cid, N, C), dtype=torch.float16, device="cuda") for _ in range(B)]
        ids = _profile(ctx, lib, lambda: K.compress_batch(cid, xs, bs, bs, pks, N, C, 0, update_cache=True))
        forms.add(KID_LAYER in ids)
        for i in range(B):
            same_packet(name, host(pks[i]), refs[i][0], ins[i][0], ins[i][1], f"packet batch {B} item {i}")
            same_bits(host(bs[i]), refs[i][1], f"state batch {B} item {i}")
        del xs, bs, pks
        torch.cuda.empty_cache()
    assert forms == {True, False}, "the batch of 2 was meant to leave the layer launch, the single tensor to take it"


# ---- (e) a captured graph of plain compress + decompress, replayed ----
@pytest.mark.parametrize("name,cid,param,N,C", _cases(D.GRAPH_SHAPES))
def test_graph_replay(name, cid, param, N, C):
    from compactfusion_amd import codecs as K
    x0, base = inputs(55 + N + C, N, C)
    state = dev(base)
    peer = dev(base)
    xin = torch.empty_like(state)
    pkt = torch.zeros(K.packet_halves(cid, N, C, param), dtype=torch.float16, device="cuda")
    ws = K.workspace(cid, N, C, param, 1, 0)
    comp = K.prepare_compress(cid, [state], [state], [pkt], N, C, param, update_cache=True)
    dec = K.prepare_decompress(cid, [pkt], [peer], [peer], N, C, param)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            comp([xin], side.cuda_stream)
            dec(side.cuda_stream)
    torch.cuda.synchronize()
    assert ws is not None or name == "topk"
    ostate = base.view(np.uint16).copy()
    for r in range(2):
        x, _ = inputs(900 + 31 * r + N, N, C)
        xin.copy_(dev(x))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        before = ostate
        p_ref, ostate = oracle(name, x, ostate.view(F16), param, N, C)
        same_packet(name, host(pkt), p_ref, x, before.view(F16), f"packet replay {r}")
        same_bits(host(state), ostate, f"sender state replay {r}")
        same_bits(host(peer), ostate, f"peer state replay {r}")


# ---- coverage: the layer form and the fallback form both ran ----
def test_coverage_layer_and_fallback_forms():
    """Over GATED_SHAPES, the gated call of 1-bit, 2-bit, int4 and int8 took the one-launch layer form (kernel id 31 alone) for some shape
    and the multi-launch fallback for another; top-k has no shape rule (its layer form is decided by the stream and the loop-back), so
    only its layer form is required.  A change to a dispatch rule that empties either path fails here."""
    seen = {}
    for name, cid, param in D.CODECS:
        if name == "topk" and param != 8:
            continue
        for N, C in D.subset(name, param, D.GATED_SHAPES):
            ids = _gated_layer(name, cid, param, N, C, B=2, NP=3, rounds=1, seed=1, check=False)
            seen.setdefault(name, set()).add(_form(ids))
    for name in ("binary", "int2", "int4", "int8"):
        assert seen[name] == {"layer", "fallback"}, (name, seen[name])
    assert "layer" in seen["topk"], seen["topk"]


def test_coverage_unaligned_tails():
    """every codec but top-k has a plain-call shape whose packet tail sections are not 16-byte aligned, and int4 / int8 one in the
    multi-launch and gated subsets (top-k's index section starts at 2*N*C/m bytes: always aligned)"""
    for name, _, param in D.CODECS:
        un = [s for s in D.shapes_for(name, param) if not D.tails_aligned(name, *s, param)]
        assert bool(un) == (name != "topk"), (name, param, un)


# ---- non-finite input (golden G16): plain (layer-capable), multi-launch and gated layer forms ----
@pytest.mark.parametrize("case", NF.cases(), ids=NF.ids())
def test_nonfinite_golden(case):
    from compactfusion_amd import _lib, codecs as K
    _, name, param, x, base, want_pkt, want_rec = case
    cid = {"int4": 3, "int8": 4, "topk": 5}[name]
    N, C = x.shape
    xd, bd = dev(x), dev(base)
    for fused in (True, False):
        K.set_fused_finalize(fused)
        pkt, nb = K.compress(cid, xd, bd, N, C, param, update_cache=True)
        rec = K.decompress(cid, pkt, bd, N, C, param)
        torch.cuda.synchronize()
        same_bits(host(pkt), want_pkt, f"packet (fused finalize {fused})")
        same_bits(host(nb), want_rec, f"sender state (fused finalize {fused})")
        same_bits(host(rec), want_rec, f"reconstruction (fused finalize {fused})")
    K.set_fused_finalize(True)
    lib = _lib.load()
    ctx = K.context(0)
    own = dev(base)
    peer = dev(base)
    pk = torch.zeros(K.packet_halves(cid, N, C, param), dtype=torch.float16, device="cuda")
    ws = K.workspace(cid, N, C, param, 1, 0)
    wsp, wsn = (None, 0) if ws is None else (ws.data_ptr(), ws.numel())
    comp = (_lib.CompItem * 1)(_lib.CompItem(xd.data_ptr(), own.data_ptr(), own.data_ptr(), pk.data_ptr()))
    gated = (_lib.DecompItem * 1)(_lib.DecompItem(pk.data_ptr(), peer.data_ptr(), peer.data_ptr()))
    sh = torch.cuda.current_stream().cuda_stream
    ids = _profile(ctx, lib, lambda: lib.cfx_compress_batch_gated(ctx, cid, N, C, param, _lib.FLAG_UPDATE_CACHE, 1, comp, 0, None, 1, gated,
                                                                  wsp, wsn, sh))
    assert lib.cfx_gate_errors(ctx) == 0
    assert ids == [KID_LAYER], ids                  # (32, 128) / (8, 1024): the layer launch
    same_bits(host(pk), want_pkt, "packet (layer)")
    same_bits(host(own), want_rec, "sender state (layer)")
    same_bits(host(peer), want_rec, "peer reconstruction (layer)")


NF_OTHER = [pytest.param(n, cid, p, N, C, id=f"{n}{p or ''}-{N}x{C}")
            for n, cid, p in (("int8", 4, 0), ("int4", 3, 0), ("topk", 5, 16), ("topk", 5, 4))
            for N, C in ((34, 264), (130, 1160), (66, 23560), (2050, 1920), (256, 136)) if D.legal(n, N, C, p)]


@pytest.mark.parametrize("name,cid,param,N,C", NF_OTHER)
def test_nonfinite_other_forms(name, cid, param, N, C):
    """NaN / +-inf deltas at shapes that take the other min/max forms (C % 16 == 8: the fused statistics + finalize launch; CB = 47: no
    in-launch finalize; 2050 rows: the tall layer form) and whose packet tails are unaligned: bit for bit against the oracle, which golden
    G16 pins to the reference"""
    from compactfusion_amd import codecs as K
    x, base = inputs(77 + N + C, N, C)
    rng = np.random.default_rng(N + C)
    for k, v in enumerate((np.nan, np.inf, -np.inf, np.nan)):
        r, c = rng.integers(0, N, 3), rng.integers(0, C, 3)
        x[r, c] = v
    x[0, 0] = base[0, 0] = np.inf                       # inf - inf
    x[N - 1, C - 1] = np.nan
    pkt_ref, nb_ref = oracle(name, x, base, param, N, C)
    xd, bd = dev(x), dev(base)
    for fused in (True, False):
        K.set_fused_finalize(fused)
        pkt, nb = K.compress(cid, xd, bd, N, C, param, update_cache=True)
        rec = K.decompress(cid, pkt, bd, N, C, param)
        torch.cuda.synchronize()
        same_bits(host(pkt), pkt_ref, f"packet (fused finalize {fused})")
        same_bits(host(nb), nb_ref, f"sender state (fused finalize {fused})")
        same_bits(host(rec), nb_ref, f"reconstruction (fused finalize {fused})")
