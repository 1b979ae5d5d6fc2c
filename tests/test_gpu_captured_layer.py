"""The block-local codecs' layer launch as ONE launch under hipGraph capture (include/cfx.h, cfx_set_captured_layer) on the GPU (-m gpu):
a captured layer call on a private gate slot, replayed between eager launches of the same context, against the families' numpy
contracts (tests/*_contract.py, oracle/ref_np.py for top-k) - packets as whole byte strings, sender and peer states bit for bit, no gate
error - and the form proved by cfx_captured_layer_stats (and, for one family, by the kernel nodes of the captured graph).

Shapes: (4, 128) - one S and one D workgroup per tensor, divisions by 1, mostly dead lanes (top-k needs E % 1024 == 0: (8, 128)) - and
(8, 4224): E = 33792, 5 S workgroups (8192 elements each) and 3 D workgroups (16384) per tensor, both with a ragged last unit.  Two own
tensors and four loop-back reconstruction items, as in test_layer_calls_are_graph_capturable.  The graphs are chains; no test provokes a
time-out."""
import ctypes
import gc

import numpy as np
import pytest
import torch

import bf16_contract as BC
import mxint8_contract as M8
from _captured_layer import (FAMILIES, KERNEL_NODE, SHAPES, Hip, Layer, _clean_pool, _ctx, capture, dev, eager, same, set_pool,  # noqa: F401
                             shape_of, stats)
from _gpu_codec import host

pytestmark = pytest.mark.gpu


# ---- 1: the gated call and the p2p layer op, one capture, six replays between eager launches -------------------------------------------
@pytest.mark.parametrize("op", ["gated", "p2p_layer"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fam", sorted(FAMILIES))
def test_captured_layer_call_replays_as_one_launch(fam, shape, op):
    N, C = shape_of(fam, shape)
    set_pool(4)
    L = Layer(fam, N, C, seed=1000 + N, op=op)
    side = torch.cuda.Stream()
    try:
        eager(side, L, "eager launch before the capture")
        s0 = stats()
        graph = capture(side, L.call)
        L.check("capture must not execute")
        s1 = stats()
        assert (s1[0] - s0[0], s1[1] - s0[1], s1[2]) == (1, 0, 3), (s0, s1)
        for rep in range(6):
            L.step()
            graph.replay()
            L.check(f"replay {rep}")
            if rep in (1, 3):
                eager(side, L, f"eager launch behind replay {rep}")
        assert stats() == s1                      # (eager launches and replays are no capture-time calls)
        del graph
    finally:
        torch.cuda.synchronize()
        L.close()


# ---- 2: two graphs of the same call from one context, replayed alternately: separate slots ---------------------------------------------
@pytest.mark.parametrize("fam", ["bb128-bf16", "mxi8-fp16", "topk8"])
def test_two_graphs_of_one_call_have_slots_of_their_own(fam):
    N, C = 8, 4224
    set_pool(2)
    L = Layer(fam, N, C, seed=7)
    side = torch.cuda.Stream()
    try:
        eager(side, L, "eager launch before the captures")
        s0 = stats()
        g1 = capture(side, L.call)
        g2 = capture(side, L.call)
        s1 = stats()
        assert (s1[0] - s0[0], s1[1] - s0[1], s1[2]) == (2, 0, 0), (s0, s1)
        for rep in range(6):
            L.step()
            (g1 if rep % 2 == 0 else g2).replay()
            L.check(f"replay {rep} (graph {1 + rep % 2})")
        L.step()
        g2.replay()                               # ... and not in lock step: graph 2 twice in a row, then graph 1 twice
        L.check("graph 2 again")
        for rep in range(2):
            L.step()
            g1.replay()
            L.check(f"graph 1, extra replay {rep}")
        del g1, g2
    finally:
        torch.cuda.synchronize()
        L.close()


# ---- 3: three layer calls - three codecs - as a linear chain in one graph ---------------------------------------------------------------
def test_three_layer_calls_in_one_graph():
    set_pool(8)
    Ls = [Layer("bb32-fp16", 8, 4224, seed=31), Layer("mxi8-bf16", 8, 4224, seed=32, op="p2p_layer"), Layer("mxfp4", 4, 128, seed=33)]
    side = torch.cuda.Stream()
    try:
        for L in Ls:
            eager(side, L, "eager launch before the capture")
        s0 = stats()
        graph = capture(side, lambda sh: [L.call(sh) for L in Ls])
        s1 = stats()
        assert (s1[0] - s0[0], s1[1] - s0[1], s1[2]) == (3, 0, 5), (s0, s1)
        for rep in range(4):
            for L in Ls:
                L.step()
            graph.replay()
            for L in Ls:
                L.check(f"replay {rep}")
            if rep == 1:
                eager(side, Ls[0], "eager launch between replays")
        del graph
    finally:
        torch.cuda.synchronize()
        for L in Ls:
            L.close()


# ---- 4: a pool of 2 and three captured calls: the third takes the sequence; release, and a new capture takes a slot again -------------
def test_pool_of_two_third_call_takes_the_sequence_and_release():
    lib, ctx = _ctx()
    set_pool(2)
    Ls = [Layer("i2b32-bf16", 8, 4224, seed=41 + i) for i in range(3)]
    side = torch.cuda.Stream()
    try:
        s0 = stats()
        graphs = []
        for i, L in enumerate(Ls):
            graphs.append(capture(side, L.call))
            s = stats()
            assert (s[0] - s0[0], s[1] - s0[1], s[2]) == ((i + 1, 0, 1 - i) if i < 2 else (2, 1, 0)), (i, s0, s)
        assert lib.cfx_set_captured_layer(ctx, 3) == -2          # slots are handed out: no change of the pool
        assert lib.cfx_set_captured_layer(ctx, 2) == 0           # (the same size again changes nothing)
        for rep in range(3):
            for L, g in zip(Ls, graphs):
                L.step()
                g.replay()
                L.check(f"replay {rep}")
        del graphs, g
        gc.collect()
        torch.cuda.synchronize()
        assert lib.cfx_captured_layer_release(ctx) == 0
        assert stats()[2] == 2
        s2 = stats()
        graph = capture(side, Ls[2].call)
        s3 = stats()
        assert (s3[0] - s2[0], s3[1] - s2[1], s3[2]) == (1, 0, 1), (s2, s3)
        for rep in range(2):
            Ls[2].step()
            graph.replay()
            Ls[2].check(f"replay {rep} after the release")
        del graph
    finally:
        torch.cuda.synchronize()
        for L in Ls:
            L.close()


# ---- 5: what takes the sequence under capture, with identical bits ----------------------------------------------------------------------
@pytest.mark.parametrize("why", ["no_pool", "gated_launch_off", "masked_stream"])
def test_fall_backs_under_capture_take_the_sequence(why):
    lib, ctx = _ctx()
    L = Layer("bb32-fp16", 8, 4224, seed=51)
    side = torch.cuda.Stream()
    masked = ctypes.c_void_p()
    hip, held = Hip(), None
    try:
        if why != "no_pool":
            set_pool(2)
        if why == "gated_launch_off":
            assert lib.cfx_set_gated_launch(ctx, 0) == 0
        s0 = stats()
        if why == "masked_stream":
            assert lib.cfx_stream_create_masked(ctx, 0, 64, ctypes.byref(masked)) == 0
            g, ex, types = held = hip.capture(masked.value, L.call)
            assert types.count(KERNEL_NODE) == 2, types               # compress ; reconstruct
            replay = lambda: hip.launch(ex, masked.value)
        else:
            graph = capture(side, L.call)
            replay = graph.replay
        s1 = stats()
        assert (s1[0] - s0[0], s1[1] - s0[1]) == (0, 1), (why, s0, s1)
        assert s1[2] == (0 if why == "no_pool" else 2)
        for rep in range(3):
            L.step()
            replay()
            L.check(f"{why}: replay {rep}")
    finally:
        torch.cuda.synchronize()
        if held:
            hip.destroy(held[0], held[1])
        if masked.value:
            lib.cfx_stream_destroy(ctx, masked)
        L.close()


# ---- 6: the kernel nodes of the captured graph -------------------------------------------------------------------------------------------
def test_captured_graph_has_one_kernel_node_with_a_pool():
    hip = Hip()
    L = Layer("mxi8-bf16", 8, 4224, seed=61)
    side = torch.cuda.Stream()
    held = []
    try:
        sh = side.cuda_stream
        held.append(hip.capture(sh, L.call))
        assert held[0][2].count(KERNEL_NODE) > 1, held[0][2]            # no pool: compress ; reconstruct
        set_pool(1)
        held.append(hip.capture(sh, L.call))
        assert held[1][2] == [KERNEL_NODE], held[1][2]                  # a pool: the layer is ONE kernel node, and nothing else
        assert stats()[2] == 0
        for rep in range(4):
            L.step()
            hip.launch(held[rep % 2][1], sh)
            L.check(f"replay {rep} ({'one node' if rep % 2 else 'sequence'})")
    finally:
        torch.cuda.synchronize()
        for g, ex, _ in held:
            hip.destroy(g, ex)
        L.close()


# ---- 7: the Python level ------------------------------------------------------------------------------------------------------------------
def test_python_level_configure_codecs_and_layer_op():
    import compactfusion_amd
    from compactfusion_amd import codecs as K
    from compactfusion_amd.compact import xlayer
    compactfusion_amd.configure(captured_layer=8)
    K.apply_captured_layer()
    assert K.captured_layer_stats(0)["slots_free"] == 8
    N, C, bf = 8, 4224, True
    cid = M8.CID
    rng = np.random.default_rng(71)

    def rnd():
        return BC.f32_to_bf16((rng.standard_normal((N, C)) * 0.5).astype(np.float32))
    # codecs.compress_batch / decompress_batch stay capturable (they are the ungated calls: no slot is taken)
    x0, b0 = rnd(), rnd()
    xd, bd, nb, peer = dev(x0, bf), dev(b0, bf), dev(b0, bf), dev(b0, bf)
    pk = torch.zeros(K.packet_halves(cid, N, C, 0), dtype=torch.float16, device="cuda")
    side = torch.cuda.Stream()

    def pair(_sh):
        K.compress_batch(cid, [xd], [bd], [nb], [pk], N, C, 0, update_cache=True)
        K.decompress_batch(cid, [pk], [peer], [peer], N, C, 0)
    with torch.cuda.stream(side):
        pair(0)                                   # (eager first: workspaces and contexts exist before the capture)
    torch.cuda.synchronize()
    peer.copy_(bd)
    nb.copy_(bd)                                  # (the chain starts again at b0: every replay's base is the state before it)
    graph = capture(side, pair)
    want = b0
    for rep in range(3):
        x = rnd()
        xd.copy_(dev(x, bf))
        bd.copy_(nb)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        p_ref, want = M8.step(x, want, bf)
        same(host(pk), p_ref, f"compress_batch replay {rep}: packet")
        same(host(nb), want, f"compress_batch replay {rep}: sender state")
        same(host(peer), want, f"decompress_batch replay {rep}: peer state")
    assert K.captured_layer_stats(0)["slots_free"] == 8
    del graph
    # a LayerOp at world size 1 (no peers: the op is the compress of K,V with error feedback), captured and replayed == its eager result
    k0, v0, sk, sv = rnd(), rnd(), rnd(), rnd()
    kd, vd = dev(k0, bf), dev(v0, bf)
    own = [dev(sk, bf), dev(sv, bf)]
    op = xlayer.LayerOp(("captured-test", N, C, cid), cid, 0, N, C, 0, 1, None, torch.device("cuda:0"), own, [], own_update="ef")
    try:
        with torch.cuda.stream(side):
            op.run(kd, vd, side.cuda_stream)
        torch.cuda.synchronize()
        eager_states = [host(t).copy() for t in own]
        same(eager_states[0], M8.step(k0, sk, bf)[1], "LayerOp eager: K state")
        own[0].copy_(dev(sk, bf))
        own[1].copy_(dev(sv, bf))
        torch.cuda.synchronize()
        graph = capture(side, lambda sh: op.run(kd, vd, sh))
        same(host(own[0]), sk, "LayerOp: capture must not execute")
        graph.replay()
        torch.cuda.synchronize()
        for t, e, n in zip(own, eager_states, "KV"):
            same(host(t), e, f"LayerOp replay == eager: {n} state")
        del graph
    finally:
        torch.cuda.synchronize()
        op.close()
        compactfusion_amd.configure(captured_layer=0)
        K.apply_captured_layer()
