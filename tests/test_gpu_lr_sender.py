"""The low-rank SENDER's three factor chains - slab-resident (csrc/cfx_lrslab.hip, one launch), Gram six-launch (csrc/cfx_lrgram.hip) and
C-space (csrc/cfx_lowrank.hip k_lr_aq / k_lr_aty / k_lr_apply2) - against the float64 contract of tests/_lr_sender_f64.py, on inputs
whose spectrum is FLAT (tests/_lr_sender_cases.py: nothing converges, so a product that loses a row split or a column tail moves U V by
10 .. 1000 times what a correct chain shows - tests/test_lr_sender_f64_host.py measures it), at the smallest shapes that take every branch
of the host's dispatch, each chain forced with cfx_set_lr_chain:

  * every case: finite packet, projection (global, worst row, worst column), orthonormality, coefficients; the sender's state equal to the
    receiver's decode of the packet bit for bit under cfx_set_lr_decode 0, 1 and 2 and inside the receiver's float64 interval
    (tests/_lr_f64_check.py); ef = False gives x itself; the same bits on a second call;
  * batches of distinct tensors, one without a base: the bits of the one-tensor call whatever the batch (xcd_group on and off);
  * rank-deficient residuals and x == base; LOW_RANK_Q: the packet is the int4 oracle's of the plain call's factors, byte for byte;
  * the decaying spectrum of tests/test_gpu_lowrank_slab.py on every chain with its 3e-3.

Every test prints the ratio of each contract item to its bound (`-s` shows them; docs/DESIGN_DETAIL.md 3a has the table)."""
import numpy as np
import pytest
import torch

import _lr_cases as LC
import _lr_f64_check as RW
import _lr_sender_cases as SC
import _lr_sender_f64 as W

pytestmark = pytest.mark.gpu
F16 = np.float16
CHAIN_NAME = {0: "slab", 1: "gram", 2: "cspace"}


def _api():
    from compactfusion_amd import _lib, codecs as K
    return _lib.load(), K, K.context(0)


@pytest.fixture
def switches():
    """set(chain=None, decode=None): cfx_set_lr_chain / cfx_set_lr_decode on the session's one context; both back to 0 whatever happens"""
    lib, K, ctx = _api()

    def set_(chain=None, decode=None):
        if chain is not None:
            assert lib.cfx_set_lr_chain(ctx, chain) == 0
        if decode is not None:
            assert lib.cfx_set_lr_decode(ctx, decode) == 0
    try:
        yield set_
    finally:
        lib.cfx_set_lr_chain(ctx, 0)
        lib.cfx_set_lr_decode(ctx, 0)


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def compress(quant, items, N, C, r, ef=True):
    """items: (x, base or None, q0) numpy -> (packets as uint16 words, new states as fp16), numpy"""
    lib, K, ctx = _api()
    B = len(items)
    xs, bs, qs = [dev(i[0]) for i in items], [dev(i[1]) for i in items], [dev(i[2]) for i in items]
    pk = [torch.zeros(K.lr_packet_halves(quant, N, C, r), dtype=torch.float16, device="cuda") for _ in range(B)]
    nb = [torch.zeros(N, C, dtype=torch.float16, device="cuda") for _ in range(B)]
    K.lr_compress_batch(quant, xs, bs, nb, pk, qs, N, C, r, update_cache=True, ef=ef)
    torch.cuda.synchronize()
    return [p.view(torch.int16).cpu().numpy().view(np.uint16) for p in pk], [n.cpu().numpy() for n in nb]


def decode(quant, words, base, N, C, r):
    lib, K, ctx = _api()
    out = torch.zeros(N, C, dtype=torch.float16, device="cuda")
    K.lr_decompress_batch(quant, [dev(words.view(np.int16)).view(torch.float16)], [dev(base)], [out], N, C, r)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint16), np.asarray(b).view(np.uint16))


def report(what, m):
    print(f"RATIO {what} " + " ".join(f"{k}={v:.3f}" for k, v in W.ratios(m).items()))


def contract(switches, lc, kind, N, C, r, key, what):
    """items a - f of the contract on one tensor; -> (packet words, state under decode mode 0)"""
    lib, K, ctx = _api()
    x, base, q0, ref = W.case(kind, N, C, r, key)
    switches(chain=lc, decode=0)
    (pk,), (nb,) = compress(False, [(x, base, q0)], N, C, r)
    U16, V16 = W.split(pk, N, C, r)
    m = W.check(ref, U16, V16, what)
    report(what, m)
    # f. the state is the receiver's decode of the packet, whichever form of the receiver's kernel both sides are told to run
    for mode in (0, 1, 2):
        switches(decode=mode)
        (pk_m,), (nb_m,) = compress(False, [(x, base, q0)], N, C, r)
        assert same(pk_m, pk), f"{what}: the packet changes with the decode mode {mode}, or from call to call"
        rec = decode(False, pk, base, N, C, r)
        assert same(nb_m, rec), f"{what}: sender state != receiver reconstruction under decode mode {mode}"
        RW.check(U16, V16, base, rec, f"{what} decode mode {mode}")
    switches(decode=0)
    (pk_n,), (nb_n,) = compress(False, [(x, base, q0)], N, C, r, ef=False)
    assert same(pk_n, pk) and same(nb_n, x), f"{what}: error feedback off: the state is the activation itself"
    return pk, nb


def _ids(cases):
    return [f"{c[0]}-{c[1]}-{c[2]}" for c in cases]


@pytest.mark.parametrize("N,C,r,why", SC.CSPACE, ids=_ids(SC.CSPACE))
def test_c_space_chain(switches, N, C, r, why):
    pk, nb = contract(switches, 2, "flat", N, C, r, SC.rep_of(N, C, r), f"cspace {N, C, r} [{why}]")
    if not SC.lrg_ok(N, C):
        # the automatic choice takes the same chain for a shape the N-space chains refuse
        switches(chain=0)
        x, base, q0, _ = W.case("flat", N, C, r, SC.rep_of(N, C, r))
        (pk0,), (nb0,) = compress(False, [(x, base, q0)], N, C, r)
        assert same(pk0, pk) and same(nb0, nb)


@pytest.mark.parametrize("N,C,r,why", SC.GRAM, ids=_ids(SC.GRAM))
def test_gram_six_launch_chain(switches, N, C, r, why):
    contract(switches, 1, "flat", N, C, r, SC.rep_of(N, C, r), f"gram {N, C, r} [{why}]")


@pytest.mark.parametrize("N,C,r,why", SC.SLAB, ids=_ids(SC.SLAB))
def test_slab_resident_chain(switches, N, C, r, why):
    lib, K, ctx = _api()
    contract(switches, 0, "flat", N, C, r, SC.rep_of(N, C, r), f"slab {N, C, r} [{why}]")
    assert lib.cfx_gate_errors(ctx) == 0


def test_rank_32_under_chain_1_takes_the_c_space_chain(switches):
    N, C, r = 100, 512, 32
    x, base, q0, ref = W.case("flat", N, C, r, SC.rep_of(N, C, r))
    switches(chain=1)
    (pk1,), (nb1,) = compress(False, [(x, base, q0)], N, C, r)
    W.check(ref, *W.split(pk1, N, C, r), "rank 32 under chain 1")
    switches(chain=2)
    (pk2,), (nb2,) = compress(False, [(x, base, q0)], N, C, r)
    assert same(pk1, pk2) and same(nb1, nb2)


def _batch_items(N, C, r, n):
    """n distinct tensors (draws 0 .. n - 1); item 1 has no base: its x is the residual itself"""
    items, refs = [], []
    for i in range(n):
        x, base, q0, ref = W.case("flat", N, C, r, i)
        if i == 1:
            x, base = SC.residual(x, base), None
        items.append((x, base, q0))
        refs.append(ref)
    return items, refs


BATCH_CASES = [(1, s, SC.GRAM_BATCHES) for s in SC.GRAM_BATCH_SHAPES] + [(2, s, SC.GRAM_BATCHES) for s in SC.CSPACE_BATCH_SHAPES] \
    + [(0, s, SC.SLAB_BATCHES) for s in SC.SLAB_BATCH_SHAPES]


@pytest.mark.parametrize("lc,shape,batches", BATCH_CASES, ids=[f"{CHAIN_NAME[c[0]]}-{c[1][0]}-{c[1][1]}-{c[1][2]}" for c in BATCH_CASES])
def test_batches_of_distinct_tensors_same_bits(switches, lc, shape, batches):
    """h. who sums which share of a sum depends on the launch's batch (the Gram chain deals a tensor's workgroups to its own XCDs when
    the batch divides 8); the order of the additions must not: every tensor's bits are those of its one-tensor call, on every call"""
    lib, K, ctx = _api()
    N, C, r = shape
    assert SC.chain_taken(N, C, r, lc) == CHAIN_NAME[lc]
    items, refs = _batch_items(N, C, r, max(batches))
    switches(chain=lc, decode=0)
    one = [compress(False, [it], N, C, r) for it in items]
    for i, (it, ref) in enumerate(zip(items, refs)):
        pk, nb = one[i][0][0], one[i][1][0]
        U16, V16 = W.split(pk, N, C, r)
        m = W.check(ref, U16, V16, f"{CHAIN_NAME[lc]} {shape} tensor {i}")
        report(f"{CHAIN_NAME[lc]} {shape} tensor {i}", m)
        rec = decode(False, pk, it[1], N, C, r)                        # (no base: the decode of the packet alone)
        assert same(nb, rec)
        RW.check(U16, V16, it[1], rec, f"{shape} tensor {i}")
    for B in batches:
        for call in range(2):
            pks, nbs = compress(False, items[:B], N, C, r)
            for i in range(B):
                assert same(pks[i], one[i][0][0]) and same(nbs[i], one[i][1][0]), f"batch {B} tensor {i} call {call}: bits differ"
    assert lib.cfx_gate_errors(ctx) == 0


@pytest.mark.parametrize("form,N,C,r,chains", SC.DEFICIENT, ids=[f"{c[0]}-{c[1]}-{c[2]}-{c[3]}" for c in SC.DEFICIENT])
def test_rank_deficient_residuals(switches, form, N, C, r, chains):
    """e. rank(x - base) < r: the projection is the residual itself, a direction is kept as a unit column or dropped as zeros in both
    factors; x == base: an all-zero packet and an unchanged state"""
    x, base, q0, ref = W.case("deficient", N, C, r, form)
    for lc in chains:
        assert SC.chain_taken(N, C, r, lc) == CHAIN_NAME[lc]
        switches(chain=lc, decode=0)
        what = f"{form} {N, C, r} {CHAIN_NAME[lc]}"
        (pk,), (nb,) = compress(False, [(x, base, q0)], N, C, r)
        U16, V16 = W.split(pk, N, C, r)
        m = W.measure(ref, U16, V16)
        print(f"{what}: kept {int(U16.astype(bool).any(0).sum())} of {r} directions (rank {ref.rankA}): {m}")
        assert not W.failures(m), f"{what}: {W.failures(m)}"
        assert same(nb, decode(False, pk, base, N, C, r))
        if form == "zero":
            assert not pk.view(F16).astype(bool).any() and same(nb, base)


@pytest.mark.parametrize("N,C,r,lc", SC.QUANT, ids=[f"{CHAIN_NAME[c[3]]}-{c[0]}-{c[1]}-{c[2]}" for c in SC.QUANT])
def test_quantised_packet_is_the_oracle_of_the_plain_factors(switches, N, C, r, lc):
    """g. in every chain `quantized` only redirects the store of the same fp16 factors (to the workspace, V transposed) for the int4
    factor quantiser: the LOW_RANK_Q packet is the pinned int4 oracle's of the LOW_RANK packet's factors, byte for byte, and the state
    is the receiver's decode of it"""
    assert SC.chain_taken(N, C, r, lc) == CHAIN_NAME[lc]
    x, base, q0, ref = W.case("flat", N, C, r, SC.rep_of(N, C, r))
    switches(chain=lc, decode=0)
    (pk,), _ = compress(False, [(x, base, q0)], N, C, r)
    U16, V16 = W.split(pk, N, C, r)
    W.check(ref, U16, V16, f"plain {N, C, r}")
    (pq,), (nbq,) = compress(True, [(x, base, q0)], N, C, r)
    want = LC.q_packet(U16, V16)
    assert np.array_equal(pq.view(np.uint8), want), f"{np.count_nonzero(pq.view(np.uint8) != want)} of {want.size} bytes differ"
    assert same(nbq, decode(True, pq, base, N, C, r))
    (pq2,), (nbq2,) = compress(True, [(x, base, q0)], N, C, r)
    assert same(pq2, pq) and same(nbq2, nbq)


@pytest.mark.parametrize("N,C,r,lc", SC.GRADED, ids=[f"{CHAIN_NAME[c[3]]}-{c[0]}-{c[1]}-{c[2]}" for c in SC.GRADED])
def test_decaying_spectrum_keeps_its_bound(switches, N, C, r, lc):
    """the ill-conditioned input (sigma_k = 0.7^k, 0.85^k above rank 16): 3e-3 and 5e-3 as tests/test_gpu_lowrank_slab.py asks - the case
    that sees an iteration lost, which a flat spectrum cannot"""
    assert SC.chain_taken(N, C, r, lc) == CHAIN_NAME[lc]
    contract(switches, lc, "graded", N, C, r, N + C + r, f"graded {CHAIN_NAME[lc]} {N, C, r}")
