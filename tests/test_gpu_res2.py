"""Second-order residual inside the 1-bit and 2-bit codec launches, on the GPU (-m gpu): cfx_compress_batch_res2 /
cfx_decompress_batch_res2 / cfx_plan_set_second_order against the contract (tests/res2_contract.py: the pinned oracle composed) AND
against the four-launch composition run on the same device (cfx_residual2_delta ; codec with base NULL ; decode ; cfx_residual2_update).
Packets as byte strings, both states - every comparison is of bits, there are no tolerances.  Shapes: tests/_domain_cases.py."""
import ctypes

import numpy as np
import pytest
import torch

import _dist_workers as W
import _domain_cases as D
import res2_contract as RC
from oracle import c_oracle as CO
from oracle import ref_np as R

pytestmark = pytest.mark.gpu

F16 = np.float16
BIG = 4 << 20
CODECS = [("binary", 1), ("int2", 2)]


def dev(a16):
    return torch.from_numpy(np.ascontiguousarray(a16).view(np.int16)).view(torch.float16).cuda()


def host(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def same(a, b, what):
    a, b = np.asarray(a).view(np.uint16).reshape(-1), np.asarray(b).view(np.uint16).reshape(-1)
    assert a.size == b.size, (what, a.size, b.size)
    ne = a != b
    assert not ne.any(), f"{what}: {int(ne.sum())}/{a.size} halves differ (first at {int(np.argmax(ne))})"


def inputs(seed, N, C):
    """(x, base, delta_base) bits as two WARMUP steps leave them: three consecutive steps of a drift sequence"""
    x0, x1, x2 = (t.numpy().reshape(N, C) for t in W.drift(seed, (N, C), 3))
    return x2.view(np.uint16).copy(), x1.view(np.uint16).copy(), (x1 - x0).astype(F16).view(np.uint16)


def contract(name, x, base, dbase, decay):
    N, C = x.shape
    if N * C <= BIG:
        return RC.compress(name, x, base, dbase, decay)
    CO.set_num_threads(16)                                  # (above 4M elements: the codec step by the C oracle)
    dd = R.residual2_delta(x.view(F16), base.view(F16), dbase.view(F16))
    pkt, recv = CO.compress(name, dd, None, N, C, 0, update=True)
    nb, nd = R.residual2_update(base.view(F16), dbase.view(F16), np.asarray(recv).view(F16).reshape(N, C), decay)
    return np.asarray(pkt).view(np.uint16).reshape(-1), R.bits(nb), R.bits(nd)


def composition(cid, xd, bd, dd_, decay, N, C):
    """today's four launches on the device: (packet, new_base, new_delta)"""
    from compactfusion_amd import codecs as K
    dd = torch.empty_like(xd)
    K.residual2_delta(xd, bd, dd_, dd)
    pkt, _ = K.compress(cid, dd, None, N, C, update_cache=False)
    recv = K.decompress(cid, pkt, None, N, C)
    nb, nd = torch.empty_like(bd), torch.empty_like(dd_)
    K.residual2_update(bd, dd_, recv, nb, nd, decay)
    return pkt, nb, nd


def fused(cid, xd, bd, dd_, decay, N, C, inplace):
    """(packet, sender base, sender delta, receiver base, receiver delta, recon alone) of the fused calls"""
    from compactfusion_amd import codecs as K
    pkt = torch.zeros(K.packet_halves(cid, N, C), dtype=torch.float16, device="cuda")
    rb, rd = bd.clone(), dd_.clone()
    rec_only = torch.empty_like(bd)
    if inplace:
        sb, sd = bd.clone(), dd_.clone()
        K.compress_batch_res2(cid, [xd], [sb], [sd], [sb], [sd], [pkt], N, C, decay)
        K.decompress_batch_res2(cid, [pkt], [rb], [rd], [rec_only], [None], N, C, decay)          # new_delta NULL: the reconstruction alone
        K.decompress_batch_res2(cid, [pkt], [rb], [rd], [rb], [rd], N, C, decay)
        return pkt, sb, sd, rb, rd, rec_only
    sb, sd = torch.empty_like(bd), torch.empty_like(dd_)
    K.compress_batch_res2(cid, [xd], [bd], [dd_], [sb], [sd], [pkt], N, C, decay)
    ob, od = torch.empty_like(bd), torch.empty_like(dd_)
    K.decompress_batch_res2(cid, [pkt], [rb], [rd], [rec_only], [None], N, C, decay)
    K.decompress_batch_res2(cid, [pkt], [rb], [rd], [ob], [od], N, C, decay)
    return pkt, sb, sd, ob, od, rec_only


def check(name, cid, x, base, dbase, decay, inplace, tag, against_composition=True):
    N, C = x.shape
    want_pkt, want_b, want_d = contract(name, x, base, dbase, decay)
    xd, bd, dd_ = dev(x), dev(base), dev(dbase)
    pkt, sb, sd, rb, rd, rec = fused(cid, xd, bd, dd_, decay, N, C, inplace)
    torch.cuda.synchronize()
    same(host(pkt), want_pkt, f"{tag}: packet vs contract")
    for got, what in ((sb, "sender base"), (rb, "receiver base"), (rec, "recon with new_delta NULL")):
        same(host(got), want_b, f"{tag}: {what} vs contract")
    for got, what in ((sd, "sender delta"), (rd, "receiver delta")):
        same(host(got), want_d, f"{tag}: {what} vs contract")
    same(host(bd), base, f"{tag}: the caller's base is untouched")
    same(host(dd_), dbase, f"{tag}: the caller's delta_base is untouched")
    if against_composition:
        cp, cb, cd = composition(cid, xd, bd, dd_, decay, N, C)
        torch.cuda.synchronize()
        assert host(pkt).tobytes() == host(cp).tobytes(), f"{tag}: packet vs the four-launch composition"
        same(host(sb), host(cb), f"{tag}: base vs the composition")
        same(host(sd), host(cd), f"{tag}: delta vs the composition")


@pytest.fixture(autouse=True)
def _defaults():
    from compactfusion_amd import codecs as K
    yield
    K.set_fused_finalize(True)
    K.set_rows_per_tile(0)


def _cases(pool=None):
    out = []
    for name, cid in CODECS:
        shapes = D.shapes_for(name) if pool is None else D.subset(name, 0, pool)
        out += [pytest.param(name, cid, N, C, id=f"{name}-{N}x{C}") for N, C in shapes]
    return out


# ---- every shape of the domain, in place and out of place -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cid,N,C", _cases())
def test_shapes(name, cid, N, C):
    x, base, dbase = inputs(N * 131 + C, N, C)
    check(name, cid, x, base, dbase, 0.5, True, "in place")
    check(name, cid, x, base, dbase, 0.3, False, "out of place", against_composition=N * C <= BIG)
    # update_cache off: the packet alone
    from compactfusion_amd import codecs as K
    bd, dd_ = dev(base), dev(dbase)
    pkt = torch.zeros(K.packet_halves(cid, N, C), dtype=torch.float16, device="cuda")
    K.compress_batch_res2(cid, [dev(x)], [bd], [dd_], [None], [None], [pkt], N, C, 0.5, update_cache=False)
    torch.cuda.synchronize()
    same(host(pkt), contract(name, x, base, dbase, 0.5)[0], "packet (update_cache off)")
    same(host(bd), base, "base (update_cache off)")
    same(host(dd_), dbase, "delta_base (update_cache off)")


# ---- the multi-launch forms: in-launch finalize off, every rows-per-tile override -----------------------------------------------------------
@pytest.mark.parametrize("name,cid,N,C", _cases(D.FINALIZE_OFF))
def test_finalize_off(name, cid, N, C):
    from compactfusion_amd import codecs as K
    x, base, dbase = inputs(N * 7 + C, N, C)
    K.set_fused_finalize(False)
    check(name, cid, x, base, dbase, 0.5, True, "finalize off", against_composition=False)


@pytest.mark.parametrize("rows", D.ROWS_PER_TILE)
@pytest.mark.parametrize("N,C", [(129, 144), (544, 576)])
@pytest.mark.parametrize("name,cid", CODECS)
def test_rows_per_tile(name, cid, N, C, rows):
    from compactfusion_amd import codecs as K
    x, base, dbase = inputs(N + 3 * C + rows, N, C)
    for fused_finalize in (True, False):
        K.set_fused_finalize(fused_finalize)
        K.set_rows_per_tile(rows)
        check(name, cid, x, base, dbase, 0.5, True, f"rows {rows} finalize {fused_finalize}", against_composition=False)


# ---- batches of distinct tensors -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [2, D.MAX_BATCH])
@pytest.mark.parametrize("name,cid,N,C", _cases(D.BATCH_SHAPES))
def test_batches(name, cid, N, C, B):
    from compactfusion_amd import codecs as K
    ins = [inputs(1000 * B + 17 * i + N + C, N, C) for i in range(B)]
    decay = 0.3
    refs = [contract(name, x, b, d, decay) for x, b, d in ins]
    xs, sb, sd = [dev(x) for x, _, _ in ins], [dev(b) for _, b, _ in ins], [dev(d) for _, _, d in ins]
    rb, rd = [t.clone() for t in sb], [t.clone() for t in sd]
    pks = [torch.zeros(K.packet_halves(cid, N, C), dtype=torch.float16, device="cuda") for _ in range(B)]
    K.compress_batch_res2(cid, xs, sb, sd, sb, sd, pks, N, C, decay)
    K.decompress_batch_res2(cid, pks, rb, rd, rb, rd, N, C, decay)
    torch.cuda.synchronize()
    for i, (p, nb, nd) in enumerate(refs):
        same(host(pks[i]), p, f"packet item {i}/{B}")
        same(host(sb[i]), nb, f"sender base item {i}/{B}")
        same(host(sd[i]), nd, f"sender delta item {i}/{B}")
        same(host(rb[i]), nb, f"receiver base item {i}/{B}")
        same(host(rd[i]), nd, f"receiver delta item {i}/{B}")


# ---- values --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cid", CODECS)
def test_zero_delta_base_is_the_first_order_call(name, cid):
    """delta_base all +0: the packet and new_base of the plain first-order call, bit for bit (dd = (x - base) - 0, pred = base + 0)"""
    from compactfusion_amd import codecs as K
    N, C = 130, 136
    x, base, _ = inputs(77, N, C)
    zero = np.zeros((N, C), np.uint16)
    check(name, cid, x, base, zero, 0.5, True, "zero delta")
    xd, bd = dev(x), dev(base)
    p1, nb1 = K.compress(cid, xd, bd, N, C, update_cache=True)
    sb, sd = bd.clone(), dev(zero)
    pkt = torch.zeros_like(p1)
    K.compress_batch_res2(cid, [xd], [sb], [sd], [sb], [sd], [pkt], N, C, 0.5)
    torch.cuda.synchronize()
    assert host(pkt).tobytes() == host(p1).tobytes()
    same(host(sb), host(nb1), "new_base == the first-order state")


@pytest.mark.parametrize("decay", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("name,cid", CODECS)
def test_values_signed_zeros_large_residuals_and_decays(name, cid, decay):
    N, C = 66, 520
    x, base, dbase = inputs(5 + int(10 * decay), N, C)
    rng = np.random.default_rng(9)
    # signed zeros in delta_base (and in base, x): -0 and +0 scattered over a quarter of the elements
    m = rng.random((N, C))
    dbase = np.where(m < 0.125, np.uint16(0x8000), np.where(m < 0.25, np.uint16(0), dbase)).astype(np.uint16)
    x = np.where(m > 0.95, np.uint16(0x8000), x).astype(np.uint16)
    check(name, cid, x, base, dbase, decay, True, f"signed zeros, decay {decay}")
    # |dd| near 60000 in one element of twenty (x near +-30000, base near -+20000, delta_base near -+10000: every step finite in fp16; the
    # tile partials leave their 32-bit words); the rest stays drift-sized, so that the scales - and 2 x threshold - stay finite as well
    big = rng.random((N, C)) < 0.05
    s = np.where(rng.random((N, C)) < 0.5, 1.0, -1.0)
    xb = np.where(big, (s * (29000 + 1000 * rng.random((N, C)))).astype(F16), x.view(F16))
    bb = np.where(big, (-s * (19000 + 1000 * rng.random((N, C)))).astype(F16), base.view(F16))
    db = np.where(big, (-s * (9500 + 500 * rng.random((N, C)))).astype(F16), dbase.view(F16))
    dd = R.residual2_delta(xb, bb, db)
    assert np.isfinite(dd).all() and 57000 < np.abs(dd.astype(np.float32)).max() < 65504
    want = contract(name, xb.view(np.uint16), bb.view(np.uint16), db.view(np.uint16), decay)
    assert np.isfinite(want[1].view(F16)).all() and np.isfinite(want[2].view(F16)).all()
    check(name, cid, xb.view(np.uint16), bb.view(np.uint16), db.view(np.uint16), decay, False, f"|dd| near 60000, decay {decay}")


# ---- a CU-masked stream (32 CUs: 4 rows in flight in the 1-bit reconstruction, the lane's statistics tiles) -----------------------------
@pytest.mark.parametrize("name,cid", CODECS)
def test_cu_masked_stream(name, cid):
    from compactfusion_amd import _lib, codecs as K
    lib, ctx = _lib.load(), K.context(0)
    N, C = 544, 576
    x, base, dbase = inputs(321, N, C)
    want_pkt, want_b, want_d = contract(name, x, base, dbase, 0.5)
    h = ctypes.c_void_p()
    assert lib.cfx_stream_create_masked(ctx, 0, 32, ctypes.byref(h)) == 0
    try:
        s = torch.cuda.ExternalStream(h.value)
        xd, sb, sd = dev(x), dev(base), dev(dbase)
        rb, rd = sb.clone(), sd.clone()
        pkt = torch.zeros(K.packet_halves(cid, N, C), dtype=torch.float16, device="cuda")
        torch.cuda.synchronize()
        K.compress_batch_res2(cid, [xd], [sb], [sd], [sb], [sd], [pkt], N, C, 0.5, stream=s)
        K.decompress_batch_res2(cid, [pkt], [rb], [rd], [rb], [rd], N, C, 0.5, stream=s)
        torch.cuda.synchronize()
        same(host(pkt), want_pkt, "packet")
        same(host(sb), want_b, "sender base")
        same(host(sd), want_d, "sender delta")
        same(host(rb), want_b, "receiver base")
        same(host(rd), want_d, "receiver delta")
    finally:
        torch.cuda.synchronize()
        assert lib.cfx_stream_destroy(ctx, h) == 0


# ---- a captured graph: 3 replays between eager calls of the same context ----------------------------------------------------------------
@pytest.mark.parametrize("name,cid,N,C", _cases(D.GRAPH_SHAPES))
def test_graph_replay(name, cid, N, C):
    from compactfusion_amd import codecs as K
    decay = 0.5
    xs = [t.numpy().reshape(N, C).view(np.uint16).copy() for t in W.drift(55 + N + C, (N, C), 7)]
    b0, d0 = xs[1], (xs[1].view(F16) - xs[0].view(F16)).astype(F16).view(np.uint16)
    sb, sd = dev(b0), dev(d0)
    rb, rd = sb.clone(), sd.clone()
    xin = torch.empty_like(sb)
    pkt = torch.zeros(K.packet_halves(cid, N, C), dtype=torch.float16, device="cuda")
    side = torch.cuda.Stream()
    ws = K.workspace(cid, N, C, 0, 1, 0, side.cuda_stream)

    def step(stream):
        K.compress_batch_res2(cid, [xin], [sb], [sd], [sb], [sd], [pkt], N, C, decay, stream=stream, ws=ws)
        K.decompress_batch_res2(cid, [pkt], [rb], [rd], [rb], [rd], N, C, decay, stream=stream)
    ob, od = b0, d0

    def advance(x, how, what):
        nonlocal ob, od
        xin.copy_(dev(x))
        torch.cuda.synchronize()
        how()
        torch.cuda.synchronize()
        p, ob, od = contract(name, x, ob, od, decay)
        same(host(pkt), p, f"packet {what}")
        for got, want, w in ((sb, ob, "sender base"), (sd, od, "sender delta"), (rb, ob, "receiver base"), (rd, od, "receiver delta")):
            same(host(got), want, f"{w} {what}")
    advance(xs[2], lambda: step(side), "eager before the capture")
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    snap = [t.clone() for t in (sb, sd, rb, rd)]
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            step(side)
    torch.cuda.synchronize()
    for t, s_ in zip((sb, sd, rb, rd), snap):       # (a capture runs nothing; restore in case the runtime did)
        t.copy_(s_)
    for r in range(3):
        advance(xs[3 + r], graph.replay, f"replay {r}")
    advance(xs[6], lambda: step(side), "eager after the replays")


# ---- plan ops ------------------------------------------------------------------------------------------------------------------------
def _kernel_ids(lib, ctx):
    ids, ms = (ctypes.c_int * 4096)(), (ctypes.c_float * 4096)()
    n = lib.cfx_profile_read(ctx, ids, ms, 4096)
    return [ids[i] for i in range(n)]


@pytest.mark.parametrize("N,C", [(64, 512), (129, 384)])
@pytest.mark.parametrize("name,cid", CODECS)
def test_plan_compress_and_decompress_ops(name, cid, N, C):
    """compress ; set_second_order and decompress ; set_second_order, replayed 4 times (and once more through a copied op)"""
    from compactfusion_amd import _lib, codecs as K
    lib, ctx = _lib.load(), K.context(0)
    decay = 0.5
    xs = [t.numpy().reshape(N, C).view(np.uint16).copy() for t in W.drift(91 + N, (N, C), 8)]
    b0, d0 = xs[1], (xs[1].view(F16) - xs[0].view(F16)).astype(F16).view(np.uint16)
    sb, sd = [dev(b0), dev(b0)], [dev(d0), dev(d0)]
    rb, rd = [dev(b0), dev(b0)], [dev(d0), dev(d0)]
    xin = [torch.empty_like(sb[0]) for _ in range(2)]
    pk = [torch.zeros(K.packet_halves(cid, N, C), dtype=torch.float16, device="cuda") for _ in range(2)]
    ws = K.workspace(cid, N, C, 0, 2, 0)
    plan = lib.cfx_plan_create(ctx)
    c = (_lib.CompItem * 2)(*[_lib.CompItem(xin[i].data_ptr(), sb[i].data_ptr(), sb[i].data_ptr(), pk[i].data_ptr()) for i in range(2)])
    d = (_lib.DecompItem * 2)(*[_lib.DecompItem(pk[i].data_ptr(), rb[i].data_ptr(), rb[i].data_ptr()) for i in range(2)])
    c2 = (_lib.SecondItem * 2)(*[_lib.SecondItem(sd[i].data_ptr(), sd[i].data_ptr()) for i in range(2)])
    r2 = (_lib.SecondItem * 2)(*[_lib.SecondItem(rd[i].data_ptr(), rd[i].data_ptr()) for i in range(2)])
    assert lib.cfx_plan_add_compress(plan, cid, N, C, 0, _lib.FLAG_UPDATE_CACHE, 2, c, ws.data_ptr(), ws.numel()) == 0
    assert lib.cfx_plan_add_decompress(plan, cid, N, C, 0, 2, d) == 1
    assert lib.cfx_plan_flags(plan, 2) and lib.cfx_plan_add_flag_set(plan, 0) == 2
    assert lib.cfx_plan_set_second_order(plan, 2, 0, None, 0, None, decay) == -5                # a flag op
    assert lib.cfx_plan_set_second_order(plan, 0, 2, c2, 0, None, decay) == 0
    assert lib.cfx_plan_set_second_order(plan, 1, 0, None, 2, r2, decay) == 0
    assert lib.cfx_plan_finalize(plan) == 0
    other = lib.cfx_plan_create(ctx)
    assert lib.cfx_plan_copy_op(other, plan, 0) == 0 and lib.cfx_plan_copy_op(other, plan, 1) == 1
    sh = torch.cuda.current_stream().cuda_stream
    ob = [b0, b0]
    od = [d0, d0]
    for t in range(5):
        for i in range(2):
            xin[i].copy_(dev(xs[2 + t] if i == 0 else xs[7 - t]))
        torch.cuda.synchronize()
        p = plan if t < 4 else other
        assert lib.cfx_plan_run_pipelined(p, 0, 2, sh) == 0 if t == 1 else lib.cfx_plan_run(p, 0, 2, sh) == 0
        torch.cuda.synchronize()
        for i in range(2):
            want_p, ob[i], od[i] = contract(name, xs[2 + t] if i == 0 else xs[7 - t], ob[i], od[i], decay)
            same(host(pk[i]), want_p, f"packet run {t} item {i}")
            same(host(sb[i]), ob[i], f"sender base run {t} item {i}")
            same(host(sd[i]), od[i], f"sender delta run {t} item {i}")
            same(host(rb[i]), ob[i], f"receiver base run {t} item {i}")
            same(host(rd[i]), od[i], f"receiver delta run {t} item {i}")
    assert lib.cfx_gate_errors(ctx) == 0
    lib.cfx_plan_destroy(other)
    lib.cfx_plan_destroy(plan)


@pytest.mark.parametrize("N,C", [(64, 512), (129, 384)])
@pytest.mark.parametrize("name,cid", CODECS)
def test_p2p_exchange_layer_op_looped_back(name, cid, N, C):
    """xlayer.LayerOp with second-order states on the peer-to-peer transport, 8 logical ranks looped back: 4 executions (both packet
    parities used and reused); own and peers' base and delta_base == the contract; no codec launch with id 25 / 26 / 31, one
    reconstruction launch per execution."""
    from compactfusion_amd import _lib, codecs as K
    from compactfusion_amd.compact import xlayer
    lib, ctx = _lib.load(), K.context(0)
    WL, decay = 8, 0.5
    xk = [t.numpy().reshape(N, C).view(np.uint16).copy() for t in W.drift(201 + N, (N, C), 6)]
    xv = [t.numpy().reshape(N, C).view(np.uint16).copy() for t in W.drift(301 + N, (N, C), 6)]

    def first(xs):
        return xs[1], (xs[1].view(F16) - xs[0].view(F16)).astype(F16).view(np.uint16)
    (kb0, kd0), (vb0, vd0) = first(xk), first(xv)
    xlayer.set_p2p_loopback(True)
    try:
        own, own2 = [dev(kb0), dev(vb0)], [dev(kd0), dev(vd0)]
        peers = [(r, dev(kb0), dev(vb0)) for r in range(1, WL)]
        peer2 = [(dev(kd0), dev(vd0)) for _ in range(1, WL)]
        op = xlayer.LayerOp(("res2-test", N, C, cid), cid, 0, N, C, 0, WL, None, torch.device("cuda:0"), own, peers, own_update="ef",
                            own_second=own2, peer_second=peer2, decay=decay)
        assert op.transport == "p2p"
        sh = torch.cuda.current_stream().cuda_stream
        ob, od = [kb0, vb0], [kd0, vd0]
        for t in range(4):
            kx, vx = dev(xk[2 + t]), dev(xv[2 + t])
            torch.cuda.synchronize()
            assert lib.cfx_profile_enable(ctx, 4096, 0xffffffff, 1) == 0
            op.run(kx, vx, sh)
            torch.cuda.synchronize()
            ids = _kernel_ids(lib, ctx)
            lib.cfx_profile_enable(ctx, 0, 0, 1)
            assert 25 not in ids and 26 not in ids and 31 not in ids and ids.count(4 if cid == 1 else 6) == 1, ids
            for i, x in enumerate((xk[2 + t], xv[2 + t])):
                _, ob[i], od[i] = contract(name, x, ob[i], od[i], decay)
                same(host(own[i]), ob[i], f"own base run {t} {'kv'[i]}")
                same(host(own2[i]), od[i], f"own delta run {t} {'kv'[i]}")
                for (r, *st), ds in zip(peers, peer2):
                    same(host(st[i]), ob[i], f"peer {r} base run {t} {'kv'[i]}")
                    same(host(ds[i]), od[i], f"peer {r} delta run {t} {'kv'[i]}")
        assert op.region.n_exec == 4
        assert lib.cfx_gate_errors(ctx) == 0
        op.close()
    finally:
        xlayer.set_p2p_loopback(False)
