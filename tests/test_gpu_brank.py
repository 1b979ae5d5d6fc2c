"""The 1-bit codec with rank-K scales through its C-ABI - cfx_binary_rank_compress_batch / cfx_binary_rank_decompress_batch - over the
domain the entry points accept (any N, C % 8 == 0 with N C / 8 even, ANY rank 1 .. 32, batch 1 .. 16, base NULL, CFX_FLAG_NO_EF, no
CFX_FLAG_UPDATE_CACHE), against two witnesses:

  * k_binary_rank BIT FOR BIT against tests/_brank_witness.py: the receiver on crafted packets of every value kind at every kernel shape
    of tests/_brank_cases.py (row tails, column tails, C < 512, every K % 8), the sender given the factors its own chain put into the
    packet, the flags and the null base, batches of distinct tensors;
  * the |x - base| branches of the three factor chains (k_lr_aq<RP, true, false>, k_lrg_prep, k_lrs), each forced with cfx_set_lr_chain and
    PROVED by the kernel ids the call launched, at odd and even ranks of every RP: the fp16 factors read out of the packet against the
    float64 contract of tests/_lr_sender_f64.py on |fp16(x - base)| - projection (global, worst row, worst column), orthonormality,
    coefficients, with the witness's own bounds - on the scattered-block input whose |.| has a flat spectrum (tests/test_brank_host.py
    shows a |.| lost on a tail, or a tile lost from a product, moves U V by 18 .. 3700 bounds);
  * the refusals of both entry points in the order the code checks them, nothing launched; the Python paths at an awkward shape.

Every chain test prints the ratio of each contract item to its bound (`-s` shows them)."""
import ctypes

import numpy as np
import pytest
import torch

import _brank_cases as BC
import _brank_witness as BW
import _lr_sender_cases as SC
import _lr_sender_f64 as W

pytestmark = pytest.mark.gpu
F16 = np.float16
FILL = 0x7E5A                 # a NaN pattern: what a buffer holds before the call
UPD, NO_EF = 1, 2
KID_EF, KID_DEQUANT, KID_PREP, KID_AQ, KID_ATY, KID_DECODE, KID_Q4 = 16, 4, 17, 18, 19, 22, 11     # include/cfx.h, cfx_profile_enable


def _api():
    from compactfusion_amd import _lib, codecs as K
    return _lib.load(), K, K.context(0)


@pytest.fixture
def chain():
    """set(lr_chain): cfx_set_lr_chain on the session's one context; back to 0 whatever happens"""
    lib, K, ctx = _api()
    try:
        yield lambda lc: lib.cfx_set_lr_chain(ctx, lc)
    finally:
        lib.cfx_set_lr_chain(ctx, 0)


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def filled(n):
    return torch.full((n,), FILL, dtype=torch.int16, device="cuda")


def _stream():
    return torch.cuda.current_stream(0).cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


_ws = {}


def workspace(N, C, K, B):
    lib, _, _ = _api()
    need = lib.cfx_binary_rank_workspace_bytes(N, C, K, B)
    assert need
    w = _ws.get("w")
    if w is None or w.numel() < need:
        w = _ws["w"] = torch.empty(need, dtype=torch.uint8, device="cuda")
    return w, need


def compress(items, N, C, K, flags=UPD, nb_buffer=True):
    """items: (x, base or None, q0) numpy -> (packets as bytes, new_base buffers as fp16) - both pre-filled with FILL"""
    from compactfusion_amd import _lib
    lib, _, ctx = _api()
    B = len(items)
    xs, bs, qs = [dev(i[0]) for i in items], [dev(i[1]) for i in items], [dev(i[2]) for i in items]
    nbytes = lib.cfx_binary_rank_packet_bytes(N, C, K)
    assert nbytes == BW.packet_bytes(N, C, K) != 0
    pk, nb = [filled(nbytes // 2) for _ in range(B)], [filled(N * C) for _ in range(B)]
    w, need = workspace(N, C, K, B)
    arr, qp = (_lib.CompItem * B)(), (ctypes.c_void_p * B)()
    for i in range(B):
        arr[i] = _lib.CompItem(_ptr(xs[i]), _ptr(bs[i]), _ptr(nb[i]) if nb_buffer else None, _ptr(pk[i]))
        qp[i] = qs[i].data_ptr()
    rc = lib.cfx_binary_rank_compress_batch(ctx, N, C, K, flags, B, arr, qp, w.data_ptr(), need, _stream())
    assert rc == 0, (rc, lib.cfx_last_error_string(ctx))
    torch.cuda.synchronize()
    return [p.cpu().numpy().view(np.uint8) for p in pk], [n.cpu().numpy().view(F16).reshape(N, C) for n in nb]


def decompress(items, N, C, K):
    """items: (packet bytes, base or None) -> reconstructions (fp16), the buffers pre-filled with FILL"""
    from compactfusion_amd import _lib
    lib, _, ctx = _api()
    B = len(items)
    pk, bs = [dev(np.ascontiguousarray(i[0]).view(np.int16)) for i in items], [dev(i[1]) for i in items]
    out = [filled(N * C) for _ in range(B)]
    arr = (_lib.DecompItem * B)()
    for i in range(B):
        arr[i] = _lib.DecompItem(_ptr(pk[i]), _ptr(bs[i]), _ptr(out[i]))
    rc = lib.cfx_binary_rank_decompress_batch(ctx, N, C, K, B, arr, _stream())
    assert rc == 0, (rc, lib.cfx_last_error_string(ctx))
    torch.cuda.synchronize()
    return [o.cpu().numpy().view(F16).reshape(N, C) for o in out]


def kernel_ids(fn):
    """-> (what fn returns, the kernel ids it launched)"""
    lib, _, ctx = _api()
    torch.cuda.synchronize()
    assert lib.cfx_profile_enable(ctx, 4096, 0xffffffff, 1) == 0
    try:
        res = fn()
        torch.cuda.synchronize()
        ids, ms = (ctypes.c_int * 4096)(), (ctypes.c_float * 4096)()
        n = lib.cfx_profile_read(ctx, ids, ms, 4096)
        return res, [ids[i] for i in range(n)]
    finally:
        lib.cfx_profile_enable(ctx, 0, 0, 1)


def untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint16) == FILL).all())


def q0_of(N, C, K, rep=0):
    """the start matrix: orthonormal columns, or plain gaussians where K > C allows none (only its span matters)"""
    rng = BC._rng("brank-q0", N, C, K, rep)
    if K <= C:
        return SC._q0(rng, C, K)
    q0 = np.zeros((C, SC.lr_rank_pad(K)), dtype=np.float32)
    q0[:, :K] = rng.standard_normal((C, K))
    return q0


def given_factors(what, pk, nb, x, base, N, C, K, finite=True):
    """the sender's packet and state against the witness GIVEN the factors in the packet; -> (bits, U, V)"""
    bits, U, V = BW.split(pk, N, C, K)
    assert np.array_equal(bits, BW.sign_bits(x, base)), f"{what}: sign bits"
    if finite:
        assert np.isfinite(U).all() and np.isfinite(V).all(), f"{what}: a factor section is not finite everywhere (a tail left uncopied?)"
    want = BW.apply(bits, U, V, base)
    assert BW.same(nb, want), f"{what}: state != witness on the packet's own factors, {BW.differing(nb, want)} of {N * C} elements"
    return bits, U, V


# ---- 1. the receiver, bit for bit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", BC.KIND_NAMES)
def test_receiver_bit_for_bit_on_crafted_packets(kind):
    for N, C, K in BC.KERNEL:
        v = BC.build(kind, N, C, K)
        for base in (v["base"], None):
            pk, want = BW.sender(v["x"], base, v["U"], v["V"])
            assert not np.isnan(want).any()                            # (so equality also says every element was overwritten)
            (got,), ids = kernel_ids(lambda: decompress([(pk, base)], N, C, K))
            assert ids == [KID_DEQUANT], ids
            assert BW.same(got, want), f"{kind} {N, C, K} base {base is not None}: {BW.differing(got, want)} of {N * C} elements differ"
            assert np.array_equal(got.view(np.uint16), want.view(np.uint16))


# ---- 2. the sender, bit for bit given its own factors ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "integers", "signed-zeros"])
def test_sender_bit_for_bit_given_its_own_factors(kind):
    """every kernel shape - N < 32, odd ranks, ranks past min(N, C) - takes the C-space chain; the factors are whatever it found, the rest
    is fully specified"""
    for N, C, K in BC.KERNEL:
        v = BC.build(kind, N, C, K)
        for base in (v["base"], None):
            what = f"{kind} {N, C, K} base {base is not None}"
            (pk,), (nb,) = compress([(v["x"], base, q0_of(N, C, K))], N, C, K)
            given_factors(what, pk, nb, v["x"], base, N, C, K)
            (rec,) = decompress([(pk, base)], N, C, K)
            assert np.array_equal(rec.view(np.uint16), nb.view(np.uint16)), f"{what}: receiver != sender"


def test_sender_with_nan_activations():
    """a NaN in x: its sign bit is 0 whatever the factors become, and the state is still the witness's on the packet's own factors"""
    for N, C, K in [(2, 16, 1), (8, 24, 9), (9, 512, 12), (8, 520, 9)]:
        v = BC.build("nan-x", N, C, K)
        (pk,), (nb,) = compress([(v["x"], v["base"], q0_of(N, C, K))], N, C, K)
        bits, U, V = given_factors(f"nan-x {N, C, K}", pk, nb, v["x"], v["base"], N, C, K, finite=False)
        assert not BW.unpack(bits, C)[np.isnan(v["x"])].any()
        (pk2,), (nb2,) = compress([(v["x"], v["base"], q0_of(N, C, K))], N, C, K, flags=UPD | NO_EF)
        assert np.array_equal(nb2.view(np.uint16), v["x"].view(np.uint16)) and np.array_equal(BW.split(pk2, N, C, K)[0], bits)


# ---- 3. flags and the null base ---------------------------------------------------------------------------------------------------------------
def test_flags_and_null_base():
    for N, C, K in BC.KERNEL:
        v = BC.build("random", N, C, K)
        for base in (v["base"], None):
            what = f"{N, C, K} base {base is not None}"
            it = [(v["x"], base, q0_of(N, C, K))]
            ((pk,), (nb,)), ids = kernel_ids(lambda: compress(it, N, C, K))
            assert ids[-1] == KID_EF and KID_PREP not in ids and KID_DECODE not in ids and KID_Q4 not in ids and KID_AQ in ids, ids
            assert not (pk.view(np.uint16) == FILL).all() and not untouched(nb)
            (pk1,), (nb1,) = compress(it, N, C, K, flags=UPD | NO_EF)
            assert np.array_equal(pk1, pk), f"{what}: NO_EF changes the packet"
            assert np.array_equal(nb1.view(np.uint16), v["x"].view(np.uint16)), f"{what}: NO_EF: the state is x bit for bit"
            (pk2,), (nb2,) = compress(it, N, C, K, flags=0)
            assert np.array_equal(pk2, pk) and untouched(nb2), f"{what}: no UPDATE_CACHE: same packet, new_base not written"
            (pk3,), _ = compress(it, N, C, K, flags=0, nb_buffer=False)
            assert np.array_equal(pk3, pk), f"{what}: new_base NULL without UPDATE_CACHE"
            (pk4,), (nb4,) = compress(it, N, C, K, flags=NO_EF)
            assert np.array_equal(pk4, pk) and untouched(nb4), f"{what}: NO_EF without UPDATE_CACHE writes no state"


# ---- 4. the factors: the |x - base| branches of the three chains ----------------------------------------------------------------------------
def report(what, m):
    print(f"RATIO {what} " + " ".join(f"{k}={v:.3f}" for k, v in W.ratios(m).items()))


def proves(name, ids):
    """the kernel ids of one compress call say which chain ran: the slab form is ONE launch of the chain's id, the Gram chain has a prep
    launch and products, the C-space chain no prep; k_binary_rank<QUANT> last; no decode, no int4 quantiser"""
    assert ids[-1] == KID_EF and ids.count(KID_EF) == 1 and KID_DECODE not in ids and KID_Q4 not in ids, ids
    if name == "slab":
        assert ids == [KID_PREP, KID_EF], ids
    elif name == "gram":
        assert ids.count(KID_PREP) == 1 and KID_AQ in ids and KID_ATY in ids and len(ids) > 3, ids
    else:
        assert KID_PREP not in ids and ids.count(KID_AQ) == 3 and ids.count(KID_ATY) == 3, ids


def factors_hold(chain, lc, name, x, base, q0, ref, N, C, r, what):
    lib, _, ctx = _api()
    assert chain(lc) == 0
    ((pk,), (nb,)), ids = kernel_ids(lambda: compress([(x, base, q0)], N, C, r))
    proves(name, ids)
    bits, U, V = given_factors(what, pk, nb, x, base, N, C, r)
    m = W.measure(ref, U, np.ascontiguousarray(V.T))
    report(what, m)
    assert not W.failures(m), f"{what}: " + "; ".join(W.failures(m))
    (rec,) = decompress([(pk, base)], N, C, r)
    assert np.array_equal(rec.view(np.uint16), nb.view(np.uint16)), f"{what}: receiver != sender"
    assert lib.cfx_gate_errors(ctx) == 0
    return pk, nb, m


CHAINS = BC.all_chain_cases()


@pytest.mark.parametrize("case", CHAINS, ids=lambda c: "-".join(str(v) for v in c[:5]))
def test_factor_contracts_on_the_forced_chain(chain, case):
    name, lc, N, C, r, why = case
    assert SC.chain_taken(N, C, r, lc) == name
    x, base, q0, ref = BC.chain_case(N, C, r)
    pk, nb, _ = factors_hold(chain, lc, name, x, base, q0, ref, N, C, r, f"{name} {N, C, r} [{why}]")
    auto = SC.chain_taken(N, C, r, 0)
    if auto != name:                                       # the shape the default dispatch sends elsewhere: that chain too
        factors_hold(chain, 0, auto, x, base, q0, ref, N, C, r, f"{auto} (automatic) {N, C, r}")
    elif lc != 0:                                          # ... or the same chain: the same bits
        assert chain(0) == 0
        (pk0,), (nb0,) = compress([(x, base, q0)], N, C, r)
        assert np.array_equal(pk0, pk) and np.array_equal(nb0.view(np.uint16), nb.view(np.uint16))


@pytest.mark.parametrize("form,N,C,r,chains", BC.DEFICIENT, ids=[f"{c[0]}-{c[1]}-{c[2]}-{c[3]}" for c in BC.DEFICIENT])
def test_rank_deficient_abs_residuals(chain, form, N, C, r, chains):
    """e. rank(|x - base|) < r: the projection is |x - base| itself, a direction is kept as a unit column or dropped as zeros in both
    factors; x == base: all scales 0, all bits 1, the state is base"""
    x, base, q0, ref = BC.deficient_case(form, N, C, r)
    for lc in chains:
        name = BC.CHAIN_NAME[lc]
        assert SC.chain_taken(N, C, r, lc) == name
        what = f"{form} {N, C, r} {name}"
        assert chain(lc) == 0
        ((pk,), (nb,)), ids = kernel_ids(lambda: compress([(x, base, q0)], N, C, r))
        proves(name, ids)
        bits, U, V = given_factors(what, pk, nb, x, base, N, C, r)
        m = W.measure(ref, U, np.ascontiguousarray(V.T))
        print(f"{what}: kept {int(U.astype(bool).any(0).sum())} of {r} directions (rank {ref.rankA}): {m}")
        assert not W.failures(m), f"{what}: {W.failures(m)}"
        if form == "zero":
            assert not U.astype(bool).any() and not V.astype(bool).any() and (bits == 0xFF).all()
            assert np.array_equal(nb.view(np.uint16), base.view(np.uint16))


# ---- 5. batches -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lc,N,C,r", BC.BATCH_SHAPES, ids=[f"{BC.CHAIN_NAME[c[0]]}-{c[1]}-{c[2]}-{c[3]}" for c in BC.BATCH_SHAPES])
def test_batches_of_distinct_tensors_same_bits(chain, lc, N, C, r):
    """batch 1, 3 and 16 of distinct tensors, item 1 without a base: every item's packet and state are those of its one-tensor call (the
    per-item factor pointers of k_binary_rank, the slab arena and the Gram chain's xcd_group all depend on the batch)"""
    lib, _, ctx = _api()
    assert chain(lc) == 0
    items = []
    for i in range(max(BC.BATCHES)):
        x, base, q0 = BC.scattered(N, C, r, i)
        items.append((SC.residual(x, base), None, q0) if i == 1 else (x, base, q0))
    one = []
    for i, it in enumerate(items):
        ((pk,), (nb,)), ids = kernel_ids(lambda: compress([it], N, C, r))
        proves(BC.CHAIN_NAME[lc], ids)
        given_factors(f"tensor {i}", pk, nb, it[0], it[1], N, C, r)
        one.append((pk, nb))
    assert len({o[0].tobytes() for o in one}) == len(one), "distinct tensors"
    for B in BC.BATCHES:
        pks, nbs = compress(items[:B], N, C, r)
        recs = decompress([(pks[i], items[i][1]) for i in range(B)], N, C, r)
        for i in range(B):
            assert np.array_equal(pks[i], one[i][0]), f"batch {B} tensor {i}: packet differs from the one-tensor call"
            assert np.array_equal(nbs[i].view(np.uint16), one[i][1].view(np.uint16)), f"batch {B} tensor {i}: state differs"
            assert np.array_equal(recs[i].view(np.uint16), nbs[i].view(np.uint16)), f"batch {B} tensor {i}: receiver != sender"
    assert lib.cfx_gate_errors(ctx) == 0


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_in_order_launching_nothing():
    from compactfusion_amd import _lib
    lib, _, ctx = _api()
    N, C, K = 8, 16, 3
    v = BC.build("random", N, C, K)
    x, base, q0 = dev(v["x"]), dev(v["base"]), dev(q0_of(N, C, K))
    pk, nb, out = filled(BW.packet_bytes(N, C, K) // 2), filled(N * C), filled(N * C)
    w, need = workspace(N, C, K, 16)
    need1 = lib.cfx_binary_rank_workspace_bytes(N, C, K, 1)
    good = dict(x=x.data_ptr(), base=base.data_ptr(), nb=nb.data_ptr(), pk=pk.data_ptr(), q=q0.data_ptr())

    def comp(ctx_=ctx, N=N, C=C, K=K, flags=UPD, B=1, items=True, init=True, ws=w.data_ptr(), wsn=None, **over):
        p = dict(good, **over)
        arr = (_lib.CompItem * 16)(*[_lib.CompItem(p["x"], p["base"], p["nb"], p["pk"]) for _ in range(16)])
        qp = (ctypes.c_void_p * 16)(*[p["q"]] * 16)
        wsn = lib.cfx_binary_rank_workspace_bytes(N, C, K, B) if wsn is None else wsn
        return lib.cfx_binary_rank_compress_batch(ctx_, N, C, K, flags, B, arr if items else None, qp if init else None, ws, wsn, _stream())

    def dec(ctx_=ctx, N=N, C=C, K=K, B=1, items=True, **over):
        p = dict(pk=pk.data_ptr(), base=base.data_ptr(), out=out.data_ptr())
        p.update(over)
        arr = (_lib.DecompItem * 16)(*[_lib.DecompItem(p["pk"], p["base"], p["out"]) for _ in range(16)])
        return lib.cfx_binary_rank_decompress_batch(ctx_, N, C, K, B, arr if items else None, _stream())

    def msg():
        return lib.cfx_last_error_string(ctx)

    def refused():
        # 1. null ctx / items / init_q - before anything else, whatever else is wrong
        assert comp(ctx_=None) == -1 and comp(items=False, B=0) == -1 and comp(init=False, K=0) == -1
        assert b"binary rank-K compress: null ctx/items/init_q" in msg()
        # 2. the batch - before the shape
        assert comp(B=0, C=12) == -5 and comp(B=17, K=0) == -5 and b"binary rank-K compress: batch out of range" in msg()
        # 3. the shape - before the workspace
        for bad in (dict(C=12), dict(C=0), dict(K=0), dict(K=33), dict(N=1, C=8), dict(N=3, C=24), dict(N=0), dict(N=-1)):
            assert comp(ws=None, wsn=0, **bad) == -2, bad
            assert b"binary rank-K compress: bad shape / rank (1 .. 32)" in msg()
        # 4. the workspace - before the items
        assert comp(ws=None, x=None) == -7 and comp(wsn=need1 - 1, pk=None) == -7 and b"binary rank-K compress: workspace too small" in msg()
        assert comp(B=16, wsn=need - 1) == -7
        # 5. per item: null x / packet, UPDATE_CACHE without new_base, alignment, then the chain's own check of the start matrix
        assert comp(x=None, base=good["base"] + 2) == -1 and comp(pk=None) == -1 and b"binary rank-K compress: null x/packet" in msg()
        assert comp(nb=None, x=good["x"] + 2) == -1 and b"binary rank-K compress: UPDATE_CACHE needs new_base" in msg()
        for k in ("x", "base", "nb", "pk"):
            assert comp(q=None, **{k: good[k] + 8}) == -3, k
            assert b"binary rank-K compress: pointers must be 16-byte aligned" in msg()
        assert comp(q=None) == -1 and b"null x/packet/init_q" in msg()
        assert comp(q=good["q"] + 4) == -3 and b"pointers must be 16-byte aligned" in msg()
        # the receiver
        assert dec(ctx_=None) == -1 and dec(items=False, B=0) == -1 and b"binary rank-K decompress: null ctx/items" in msg()
        assert dec(B=0, C=12) == -5 and dec(B=17, K=33) == -5 and b"binary rank-K decompress: batch out of range" in msg()
        for bad in (dict(C=12), dict(K=0), dict(K=33), dict(N=1, C=8), dict(N=3, C=24), dict(N=0)):
            assert dec(pk=None, **bad) == -2, bad
            assert b"binary rank-K decompress: bad shape / rank (1 .. 32)" in msg()
        assert dec(pk=None, out=out.data_ptr() + 2) == -1 and dec(out=None) == -1 and b"binary rank-K decompress: null packet/recon" in msg()
        for k, p in (("pk", pk), ("base", base), ("out", out)):
            assert dec(**{k: p.data_ptr() + 2}) == -3, k
            assert b"binary rank-K decompress: pointers must be 16-byte aligned" in msg()

    _, ids = kernel_ids(refused)
    assert ids == [], f"a refused call launched {ids}"
    for buf in (pk, nb, out):
        assert untouched(buf.cpu().numpy()), "a refused call wrote"
    # and the same arguments with nothing wrong run
    assert comp() == 0 and dec() == 0
    torch.cuda.synchronize()
    assert not untouched(pk.cpu().numpy()) and not untouched(nb.cpu().numpy()) and not untouched(out.cpu().numpy())
    assert np.array_equal(out.cpu().numpy(), nb.cpu().numpy())


# ---- 7. the Python paths ----------------------------------------------------------------------------------------------------------------------
def test_python_paths_at_an_awkward_shape():
    """fastpath.binary_quant_fastpath / binary_dequant_fastpath and compress_quantize's rank >= 1 pair at a row tail, a column tail past a
    512 block and an odd rank: (10, 520), rank 3.  (9, 520) has an odd number of sign-bit bytes (585): the factor sections would not be
    fp16-aligned, include/cfx.h's size functions answer 0 and every Python path says so."""
    from compactfusion_amd.compact import compress_quantize as CQ, fastpath as FP, lowrank as LR
    N, C, K = BC.PY_SHAPE
    assert (N, C, K) == (9, 520, 3) and not BC.accepted(N, C, K)
    bad = torch.zeros(N, C, dtype=torch.float16, device="cuda")
    with pytest.raises(ValueError):
        FP.binary_quant_fastpath(bad, bad, K, True)
    with pytest.raises(ValueError):
        CQ.quantize_1bit(bad, K)
    N = 10
    v = BC.build("random", N, C, K)
    x, base = dev(v["x"]), dev(v["base"])
    LR.set_init_q(torch.from_numpy(q0_of(N, C, K)[:, :K].copy()))
    try:
        packed, u, vt, nb = FP.binary_quant_fastpath(x, base, K, True)
        packed0, u0, vt0, nb0 = FP.binary_quant_fastpath(x, base, K, False)
        qp, qu, qv = CQ.quantize_1bit(x, K)
    finally:
        LR.set_init_q(None)
    assert packed.dtype == torch.uint8 and tuple(packed.shape) == (N, C // 8) and tuple(u.shape) == (N, K) and tuple(vt.shape) == (C, K)
    assert nb0 is None and torch.equal(packed0, packed) and torch.equal(u0.view(torch.int16), u.view(torch.int16)) and torch.equal(vt0.view(torch.int16), vt.view(torch.int16))
    h = lambda t: t.cpu().numpy()
    pk = BW.packet(h(packed), h(u), h(vt))
    given_factors("fastpath (10, 520, 3)", pk, h(nb), v["x"], v["base"], N, C, K)
    rec = FP.binary_dequant_fastpath(packed, u, vt, base)
    assert torch.equal(rec.view(torch.int16), nb.view(torch.int16)), "fastpath: receiver state != sender state"
    # compress_quantize: no base, V as (K, C)
    assert tuple(qp.shape) == (N, C // 8) and tuple(qu.shape) == (N, K) and tuple(qv.shape) == (K, C) and qv.is_contiguous()
    assert np.array_equal(h(qp), BW.sign_bits(v["x"], None)) and torch.isfinite(qu).all() and torch.isfinite(qv).all()
    got = CQ.dequantize_1bit(qp, qu, qv)
    want = BW.apply(h(qp), h(qu), h(qv).T, None)
    assert BW.same(h(got), want) and np.array_equal(h(got).view(np.uint16), want.view(np.uint16))
