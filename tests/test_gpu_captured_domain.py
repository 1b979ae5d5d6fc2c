"""Every one of the 26 capturable layer kernels (csrc/cfx_capture.hip k_*_layer_cap; tests/_captured_layer.py TWINS) held to its family's
value contract on the GPU (-m gpu), launched the only way it can be: captured on a private gate slot and replayed.  Packets as whole byte
strings, sender and peer states bit for bit against the family's numpy contract by the rules of the family's eager test, the family's float64
witness wherever that test runs it, no gate error, and the form proved at capture time by cfx_captured_layer_stats (one_launch + 1,
sequence + 0, one slot fewer).

  1  the value domain: every case and repetition of the family's case module at every shape of its list, one graph per parameter
  2  launch geometry: 1 S + 1 D workgroup, 2 S + 1 D with a ragged last unit, 3 S + 2 D with a short last D workgroup; batches of 1 and 16
     own tensors and reconstruction items; three 16-item layers on neighbouring slots replayed out of step; the p2p layer op
  3  flags and aliasing: update-cache off, CFX_FLAG_NO_EF, NULL bases on either item type, out-of-place outputs; refused calls take no slot
  4  cfx_gate_recover under live graphs
The graphs are chains; no test provokes a time-out."""
import pytest
import torch

import _captured_layer as H
from _captured_layer import DomainLayer, _clean_pool, capture, set_pool, stats      # noqa: F401  (the fixture is autouse here too)

pytestmark = pytest.mark.gpu

TW = H.twins()
PICK = H.pick()


def captured(L, side, pool_left):
    """capture L's call: the graph, with the form proved - one capturable launch, no sequence, one slot taken"""
    s0 = stats()
    graph = capture(side, L.call)
    s1 = stats()
    assert (s1[0] - s0[0], s1[1] - s0[1], s0[2] - s1[2], s1[2]) == (1, 0, 1, pool_left), (L.t, s0, s1)
    return graph


# ---- 1: the value domain, every twin --------------------------------------------------------------------------------------------------
_DOMAIN = H.domain_params()


def test_every_twin_keeps_a_shape():
    kept = {t.name for t, _, _ in _DOMAIN}
    assert kept == {t.name for t in TW} and len(kept) == 26, sorted({t.name for t in TW} - kept)


@pytest.mark.parametrize("t,N,C", _DOMAIN, ids=[f"{t}-{n}x{c}" for t, n, c in _DOMAIN])
def test_value_domain_every_twin(t, N, C):
    cases = t.cases(N, C)
    set_pool(1)
    L = DomainLayer(t, N, C, nb=2, npeer=3)
    side = torch.cuda.Stream()
    try:
        first = [t.build(cases[0], N, C, rep=r) for r in t.pairs(cases[0], N, C)[0]]
        L.load(first)
        graph = captured(L, side, 0)
        for i in range(2):
            H.same(H.host(L.own[i]), first[i][1], f"{t} {N}x{C}: capture must not execute")
        s1 = stats()
        replays, eager_done = 0, False
        for case in cases:
            witness = t.witnessed(case)
            for a, b in t.pairs(case, N, C):
                L.load([t.build(case, N, C, rep=r) for r in (a, b)])
                for rnd in range(2 if a == 0 else 1):          # (the second round's residual is the first round's error)
                    want = L.expect()
                    graph.replay()
                    replays += 1
                    L.check(want, f"{t} {N}x{C} case {case} rep {a} round {rnd} replay {replays}", witness)
                if not eager_done:                              # an eager launch between replays: the context's host-advanced counters move
                    eager_done = True
                    want = L.expect()
                    with torch.cuda.stream(side):
                        L.call(side.cuda_stream)
                    L.check(want, f"{t} {N}x{C} case {case}: eager launch behind replay {replays}", witness)
        assert replays == H.prescribed_replays(t, cases, N, C), (t, N, C, replays)
        assert stats() == s1
        del graph
    finally:
        torch.cuda.synchronize()
        L.close()


# ---- 2: launch geometry and the slot's edges ------------------------------------------------------------------------------------------
GEOMETRY, geometry_shape = H.GEOMETRY, H.geometry_shape        # (held to the workgroup counts they name by the CPU test of the table)


def _two_cases(t, N, C):
    return [t.build(c, N, C, rep=0) for c in (t.random_case(), t.adversarial_case())]


@pytest.mark.parametrize("kind", list(GEOMETRY))
@pytest.mark.parametrize("t", TW, ids=str)
def test_geometry_every_twin(t, kind):
    N, C = geometry_shape(t, kind)
    assert H.geometry(N, C) == GEOMETRY[kind][2:]
    set_pool(1)
    L = DomainLayer(t, N, C, nb=2, npeer=3)
    side = torch.cuda.Stream()
    try:
        ins = _two_cases(t, N, C)
        L.load(ins)
        graph = captured(L, side, 0)
        for rep, pair in enumerate((ins, ins[::-1])):
            L.load(pair)
            for rnd in range(2):
                want = L.expect()
                graph.replay()
                L.check(want, f"{t} {kind} {N}x{C} order {rep} round {rnd} replay {2 * rep + rnd}", witness=True)
        del graph
    finally:
        torch.cuda.synchronize()
        L.close()


@pytest.mark.parametrize("nb,npeer", [(1, 1), (1, 16), (16, 1), (16, 16)])
@pytest.mark.parametrize("t", PICK, ids=str)
def test_batches_of_1_and_16(t, nb, npeer):
    """CFX_MAX_BATCH own tensors and as many reconstruction items - every ticket line of the slot drawn from - and one of each"""
    N, C = H.small_shape(t)
    set_pool(1)
    L = DomainLayer(t, N, C, nb=nb, npeer=npeer)
    side = torch.cuda.Stream()
    try:
        L.load(H.batch_inputs(t, N, C, nb, seed0=H.BATCH_SEEDS[0]))
        graph = captured(L, side, 0)
        for rep in range(3):                                   # (replay 1 is a second round over replay 0's states)
            if rep == 2:
                L.load(H.batch_inputs(t, N, C, nb, seed0=H.BATCH_SEEDS[1]))
            want = L.expect()
            graph.replay()
            L.check(want, f"{t} {N}x{C} nb {nb} np {npeer} replay {rep}", witness=True)
        del graph
    finally:
        torch.cuda.synchronize()
        L.close()


ORDER = H.ORDER


@pytest.mark.parametrize("t", PICK, ids=str)
def test_three_16_item_layers_on_neighbouring_slots(t):
    """a pool of exactly 3: the three layers' slots are neighbours, and each draws from all 16 ticket lines - the last one lies directly in
    front of the next slot's arrival counter.  After EVERY replay all three layers hold what the contract says."""
    assert all(ORDER.count(k) >= 4 for k in range(3)) and any(a == b for a, b in zip(ORDER, ORDER[1:]))
    N, C = H.small_shape(t)
    set_pool(3)
    Ls = [DomainLayer(t, N, C, nb=3, npeer=16) for _ in range(3)]
    side = torch.cuda.Stream()
    try:
        graphs = []
        for k, L in enumerate(Ls):
            L.load(H.batch_inputs(t, N, C, 3, seed0=H.layer_seed(k, 0)))
            graphs.append(captured(L, side, 2 - k))
        last, done = [None] * 3, [0] * 3
        for n, k in enumerate(ORDER):
            if done[k] % 2 == 0:                                 # fresh inputs on a layer's even replays, a further round on its odd ones
                Ls[k].load(H.batch_inputs(t, N, C, 3, seed0=H.layer_seed(k, done[k])))
            done[k] += 1
            last[k] = Ls[k].expect()
            graphs[k].replay()
            for j in range(3):
                if last[j] is not None:
                    Ls[j].check(last[j], f"{t} {N}x{C} layer {j} after replay {n} (of layer {k})", witness=(j == k))
        assert stats()[2] == 0
        del graphs
    finally:
        torch.cuda.synchronize()
        for L in Ls:
            L.close()


@pytest.mark.parametrize("t", TW, ids=str)
def test_p2p_layer_op_every_twin(t):
    """the peer-to-peer exchange-layer op (no live peer): the slot's external gate, opened by the in-launch exchange"""
    N, C = geometry_shape(t, "2S-1D")
    set_pool(1)
    L = DomainLayer(t, N, C, nb=2, npeer=4, op="p2p_layer")
    side = torch.cuda.Stream()
    try:
        ins = _two_cases(t, N, C)
        L.load(ins)
        graph = captured(L, side, 0)
        for rep in range(3):
            if rep == 2:                                         # (replay 1 is a second round over replay 0's states)
                L.load(ins[::-1])
            want = L.expect()
            graph.replay()
            L.check(want, f"{t} p2p layer op {N}x{C} replay {rep}", witness=True)
        del graph
    finally:
        torch.cuda.synchronize()
        L.close()


# ---- 3: flags and aliasing under capture ----------------------------------------------------------------------------------------------
VARIANTS = {
    "update-cache-off": dict(flags=0),                                        # packet right, own state untouched, peers still reconstruct
    "no-ef": dict(flags=H.FLAG_UPDATE_CACHE | H.FLAG_NO_EF),                  # state == x
    "comp-base-null": dict(comp_base=False),                                  # the codec sees x itself
    "decomp-base-null": dict(peer_base=False),                                # recon == recv, bits verbatim
    "out-of-place": dict(in_place=False),                                     # new_base != base, recon != base: the inputs stay
}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("t", PICK, ids=str)
def test_flags_and_aliasing(t, variant):
    N, C = H.small_shape(t)
    set_pool(1)
    L = DomainLayer(t, N, C, nb=2, npeer=3, **VARIANTS[variant])
    side = torch.cuda.Stream()
    try:
        ins = H.batch_inputs(t, N, C, 2, seed0=3)
        if t.neg_zero_case():                                   # own tensor 0: a recv with -0 elements, which a +0 base would turn into +0
            ins[0] = t.build(t.neg_zero_case(), N, C)
            assert (t.recon(t.step(*ins[0])[0], None, N, C) == 0x8000).any(), (t, t.neg_zero_case())
        L.load(ins)
        graph = captured(L, side, 0)
        for rep in range(2):
            if rep:
                L.new_x([x for x, _ in H.batch_inputs(t, N, C, 2, seed0=13)])
            want = L.expect()
            pk, nbo, rec, before = want
            graph.replay()
            L.check(want, f"{t} {variant} {N}x{C} replay {rep}")
            # what the variant is there for, said once more in its own words
            if variant == "update-cache-off":
                assert nbo == [None, None]
                H.same(H.host(L.own[0]), ins[0][1], f"{t} {variant} replay {rep}: own state untouched")
            elif variant == "no-ef":
                H.same(H.host(L.own[0]), L.x[0], f"{t} {variant} replay {rep}: state == x")
            elif variant == "decomp-base-null":
                t.same_state(H.host(L.peer[0]), t.recon(pk[0], None, N, C), f"{t} {variant} replay {rep}: recon == recv")
            elif variant == "out-of-place":
                H.same(H.host(L.own[1]), ins[1][1], f"{t} {variant} replay {rep}: base unchanged")
        del graph
    finally:
        torch.cuda.synchronize()
        L.close()


@pytest.mark.parametrize("t", PICK, ids=str)
def test_refused_calls_take_no_slot(t):
    """what cfx_compress_batch_gated refuses, it refuses before any launch - under capture too: UPDATE_CACHE without new_base is
    CFX_ERR_NULL, more than CFX_MAX_BATCH reconstruction items CFX_ERR_BATCH; neither takes a slot, and the graph is the good call alone"""
    from compactfusion_amd import _lib
    N, C = H.small_shape(t)
    set_pool(2)
    L = DomainLayer(t, N, C, nb=2, npeer=3)
    side = torch.cuda.Stream()
    rcs = []
    try:
        ins = H.batch_inputs(t, N, C, 2, seed0=3)
        L.load(ins)
        bad = (_lib.CompItem * 2)(*[_lib.CompItem(L.comp[i].x, L.comp[i].base, None, L.comp[i].packet) for i in range(2)])

        def calls(sh):
            rcs.append(L.lib.cfx_compress_batch_gated(L.ctx, t.cabi, N, C, t.param, H.FLAG_UPDATE_CACHE, 2, bad, 0, None, 3, L.gated, None, 0, sh))
            rcs.append(L.lib.cfx_compress_batch_gated(L.ctx, t.cabi, N, C, t.param, H.FLAG_UPDATE_CACHE, 2, L.comp, 0, None, H.MAX_BATCH + 1,
                                                      L.gated, None, 0, sh))
            L.call(sh)
        s0 = stats()
        graph = capture(side, calls)
        s1 = stats()
        assert rcs == [H.ERR_NULL, -5], rcs
        assert (s1[0] - s0[0], s1[1] - s0[1], s1[2]) == (1, 0, 1), (s0, s1)
        want = L.expect()
        graph.replay()
        L.check(want, f"{t} {N}x{C}: the good call behind two refused ones")
        del graph
    finally:
        torch.cuda.synchronize()
        L.close()


# ---- 4: cfx_gate_recover with live graphs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b", [("bb64-fp16", "mxi8-bf16"), ("topk16", "i3b32-bf16"), ("mxfp4", "i2b64-bf16")])
def test_gate_recover_keeps_live_graphs_valid(a, b):
    """a healthy context, the default time-out, nothing provoked: cfx_gate_recover zeroes the pool - all-zero is "before launch 0" - and the
    graphs that hold the slots go on replaying bit for bit"""
    by = {t.name: t for t in TW}
    set_pool(2)
    Ls = [DomainLayer(by[n], *H.small_shape(by[n]), nb=2, npeer=3) for n in (a, b)]
    side = torch.cuda.Stream()
    try:
        for k, L in enumerate(Ls):
            L.load(H.batch_inputs(L.t, L.N, L.C, 2, seed0=H.RECOVER_SEEDS[0] + k))
        s0 = stats()
        graph = capture(side, lambda sh: [L.call(sh) for L in Ls])
        s1 = stats()
        assert (s1[0] - s0[0], s1[1] - s0[1], s1[2]) == (2, 0, 0), (s0, s1)

        def replay(what, n):
            wants = []
            for k, L in enumerate(Ls):
                if n % 2 == 0:                                   # fresh inputs on even replays, a further round on odd ones
                    L.load(H.batch_inputs(L.t, L.N, L.C, 2, seed0=H.RECOVER_SEEDS[n // 2] + k))
                wants.append(L.expect())
            graph.replay()
            for L, w in zip(Ls, wants):
                L.check(w, f"{L.t} {what} replay {n}", witness=True)
        for n in range(3):
            replay("before the recover:", n)
        assert Ls[0].lib.cfx_gate_recover(Ls[0].ctx) == 0
        assert stats() == s1                                  # (the slots stay with their graph nodes)
        for n in range(3, 6):
            replay("after the recover:", n)
            if n == 4:
                for L in Ls:
                    w = L.expect()
                    with torch.cuda.stream(side):
                        L.call(side.cuda_stream)
                    L.check(w, f"{L.t}: eager launch between replays after the recover")
        assert Ls[0].lib.cfx_gate_errors(Ls[0].ctx) == 0
        del graph
    finally:
        torch.cuda.synchronize()
        for L in Ls:
            L.close()
