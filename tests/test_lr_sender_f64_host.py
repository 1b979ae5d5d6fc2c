"""The witness of the low-rank sender's factor chains (tests/_lr_sender_f64.py) on the CPU: it accepts the float32 port of the reference
iteration on every case tests/test_gpu_lr_sender.py runs, it rejects a chain that gets ONE product wrong, and the case lists reach every
branch the restated host rules (tests/_lr_sender_cases.py) can take."""
import numpy as np
import pytest

import _lr_sender_cases as SC
import _lr_sender_f64 as W

F16 = np.float16
FLAT = SC.all_flat_cases()
SEPARATION = 4.0          # a planted fault moves the projection by at least this many times the case's bound


def _id(c):
    return "-".join(str(v) for v in c[:5] if not isinstance(v, tuple))


@pytest.mark.parametrize("case", FLAT, ids=_id)
def test_witness_accepts_the_port_and_rejects_planted_faults(case):
    chain, lc, N, C, r, why = case
    assert SC.chain_taken(N, C, r, lc) == chain, why
    x, base, q0, ref = W.case("flat", N, C, r, SC.rep_of(N, C, r))
    # what a correct chain in single precision sends: the port's factors as fp16
    Up, Vp = W._port(ref.A, q0, r)
    m = W.check(ref, Up.astype(F16), Vp.astype(F16), f"float32 port {N, C, r}")
    # the two reference distances stay where docs/DESIGN_DETAIL.md 3a has them (floor 2.5e-4 .. 3.6e-4, port below 1e-6): a bound made of
    # them cannot quietly widen with a new case
    assert 2e-4 < ref.floor[0] < 4e-4 and ref.port[0] < 1e-6, (ref.floor, ref.port)
    assert ref.proj_bound()[0] < 1e-3
    seps = {}
    for name in W.PRODUCT_FAULTS:
        f = W.faulty_factors(ref, q0, name)
        if f is None:                                     # the shape has no such branch (one column chunk, one column tile, one row split)
            continue
        mf = W.measure(ref, *f)
        assert W.failures(mf), f"{name} at {N, C, r} passes the witness: {mf}"
        seps[name] = mf["proj"][0] / mf["proj"][1]
    print(f"{chain} {N, C, r}: floor {ref.floor[0]:.2e} port {ref.port[0]:.2e} port/bound {max(W.ratios(m).values()):.2f} faults x bound "
          + ", ".join(f"{k}: {v:.1f}" for k, v in seps.items()))
    assert seps
    if (N, C, r) in SC.DROPPED:
        return
    assert min(seps.values()) >= SEPARATION, seps
    for name in W.FACTOR_FAULTS:                          # these leave the subspace alone: (d) and (b) see them
        mf = W.measure(ref, *W.faulty_factors(ref, q0, name))
        assert W.failures(mf), f"{name} at {N, C, r} passes the witness: {mf}"


def test_few_shapes_are_dropped():
    listed = {(N, C, r) for _, _, N, C, r, _ in FLAT}
    assert set(SC.DROPPED) <= listed and 10 * len(SC.DROPPED) <= len(listed)


@pytest.mark.parametrize("N,C,r,lc", SC.GRADED)
def test_witness_accepts_the_port_on_a_decaying_spectrum(N, C, r, lc):
    x, base, q0, ref = W.case("graded", N, C, r, N + C + r)
    Up, Vp = W._port(ref.A, q0, r)
    W.check(ref, Up.astype(F16), Vp.astype(F16), f"float32 port, graded {N, C, r}")


@pytest.mark.parametrize("form,N,C,r,chains", SC.DEFICIENT)
def test_witness_on_rank_deficient_residuals(form, N, C, r, chains):
    x, base, q0, ref = W.case("deficient", N, C, r, form)
    k = ref.rankA
    assert k < r and (form != "zero" or k == 0) and (form != "rank3" or k == 3)
    U = np.zeros((N, r))
    V = np.zeros((r, C))
    if k:
        U[:, :k], V[:k] = ref.Ur, ref.Vr
    W.check(ref, U.astype(F16), V.astype(F16), f"svd factors {form, N, C, r}")
    if k:
        # a dropped direction that is not all zero, a kept one that is not a unit column
        V2 = V.copy(); V2[r - 1, 0] = 1e-3
        assert W.failures(W.measure(ref, U.astype(F16), V2.astype(F16)))
        U2 = U.copy(); U2[:, 0] *= 0.5; V3 = V.copy(); V3[0] *= 2
        assert W.failures(W.measure(ref, U2.astype(F16), V3.astype(F16)))
        assert W.failures(W.measure(ref, np.zeros((N, r), F16), np.zeros((r, C), F16)))
    nan = U.astype(F16); nan[0, 0] = np.nan
    assert W.failures(W.measure(ref, nan, V.astype(F16)))


TABLE = [(776, 264, 16), (600, 136, 8), (100, 384, 16)]


@pytest.mark.parametrize("N,C,r", TABLE)
def test_a_decaying_spectrum_hides_what_a_flat_one_shows(N, C, r):
    """the measurement behind the flat input: the same fault (an A^T Y without its last N / 8 rows, or its last 8 columns' Y) moves U V
    below the 3e-3 asked on the 0.7^k input and by more than 4 x the derived bound on the flat one"""
    def moved(A, q0, fault):
        U0, V0 = W.replay(A, q0[:, :r])
        U1, V1 = W.replay(A, q0[:, :r], fault=fault)
        return W.dist(U1 @ V1, U0 @ V0)[0]
    n0, c0 = N - N // 8, C - 8
    rows = lambda nm, M, c: c["A"][:n0].T @ c["Y"][:n0] if nm == "Z1" else M
    cols = lambda nm, M, c: c["A"][:, :c0] @ c["Q"][:c0] if nm == "Y1" else M
    xg, bg, qg, refg = W.case("graded", N, C, r, N + C + r, decay=0.7)
    xf, bf, qf, reff = W.case("flat", N, C, r, 0)
    g = [moved(refg.A, qg, f) for f in (rows, cols)]
    f = [moved(reff.A, qf, f_) for f_ in (rows, cols)]
    print(f"{N, C, r}: decay 0.7 moves U V by {g[0]:.1e} (rows) {g[1]:.1e} (columns); flat by {f[0]:.1e} {f[1]:.1e}; bound {reff.proj_bound()[0]:.1e}")
    assert max(g) < W.GRADED_TOL, "the decaying input would have seen it"
    assert min(f) > SEPARATION * reff.proj_bound()[0]
    # an iteration lost altogether is what the flat input cannot see (A^T A is a multiple of the identity on its directions) and the
    # graded one can: the reason both stay
    lost = W.planted(W.LOST_ITERATION, N, C, r)[0]
    print(f"    an iteration lost: decay 0.7 {moved(refg.A, qg, lost):.1e}, flat {moved(reff.A, qf, lost):.1e}")


def test_case_lists_reach_every_branch_of_the_host_rules():
    cs = [(N, C, r) for N, C, r, _ in SC.CSPACE]
    # k_lr_aty: every number of launched row splits 1 .. LR_NS_MAX, a ragged last split among them, and one of 8 rows
    nz = {SC.aty_splits(N, C)[2] for N, C, _ in cs}
    assert nz == set(range(1, 9)), nz
    last = {N - SC.aty_splits(N, C)[1] * (SC.aty_splits(N, C)[2] - 1) for N, C, _ in cs if SC.aty_splits(N, C)[2] > 1}
    assert 8 in last and any(v % 128 for v in last)
    assert (SC.aty_splits(600, 136)[1], SC.aty_splits(776, 136)[2]) == (384, 3)
    # k_lr_aq: every (gy_, gy0_); N below, on neither side of, and past a 32-row tile; C below 32, off 32, off 256, below 1024
    assert {SC.gy(N) for N, _, _ in cs} == {(4, 4), (2, 4), (1, 2)}
    assert {N for N, _, _ in cs} >= {5, 31, 33, 100, 600, 776, 2080, 4100}
    assert {C for _, C, _ in cs} >= {8, 24, 136, 264, 520, 1032}
    assert {r for _, _, r in cs} == {2, 8, 12, 16, 18, 24, 32}
    for lc in (0, 2):
        assert all(SC.chain_taken(N, C, r, lc) == "cspace" for N, C, r in cs if not SC.lrg_ok(N, C))
    assert all(SC.chain_taken(N, C, r, 2) == "cspace" for N, C, r in cs)
    assert any(SC.lrg_ok(N, C) and SC.chain_taken(N, C, r, 0) != "cspace" for N, C, r in cs)
    # the Gram chain: every KS, the kslab range, every N of the list, both RP, xcd_group on and off
    gr = [(N, C, r) for N, C, r, _ in SC.GRAM]
    assert all(SC.chain_taken(N, C, r, 1) == "gram" for N, C, r in gr)
    assert {SC.lrg_ks(C) for _, C, _ in gr} == {2, 4, 8}
    assert {C // SC.lrg_ks(C) for _, C, _ in gr} >= {64, 192, 320}
    assert {N for N, _, _ in gr} == {32, 33, 64, 65, 100, 129, 576} and {C for _, C, _ in gr} == {128, 256, 384, 512, 640}
    assert {r for _, _, r in gr} == {2, 8, 12, 16}
    assert {bool(SC.xcd_group(b)) for b in SC.GRAM_BATCHES} == {True, False} and {SC.xcd_group(b) for b in SC.GRAM_BATCHES} == {8, 4, 0, 1}
    assert SC.chain_taken(100, 512, 32, 1) == "cspace", "rank 32 under chain 1 falls to the C-space chain"
    # the slab-resident chain
    sl = [(N, C, r) for N, C, r, _ in SC.SLAB]
    assert all(SC.chain_taken(N, C, r, 0) == "slab" for N, C, r in sl)
    assert {N for N, _, _ in sl} == {32, 33, 100, 576} and {C for _, C, _ in sl} == {512, 640} and {r for _, _, r in sl} == {2, 8, 12, 16, 24, 32}
    assert any((N * r) & 3 for N, _, r in sl)
    # on a CU-masked lane of 32 CUs the slab form does not fit
    assert SC.chain_taken(544, 3072, 8, 0, cus=32) == "gram" and SC.chain_taken(544, 3072, 8, 0) == "slab"
    # LOW_RANK_Q: every chain at every RP it is built for
    q = {(SC.chain_taken(N, C, r, lc), SC.lr_rank_pad(r)) for N, C, r, lc in SC.QUANT}
    assert q == {("cspace", 8), ("cspace", 16), ("cspace", 32), ("gram", 8), ("gram", 16), ("slab", 8), ("slab", 16), ("slab", 32)}
    assert all(N % 2 == 0 and r % 8 == 0 for N, _, r, _ in SC.QUANT)
    for N, C, r, lc in SC.GRADED:
        assert SC.chain_taken(N, C, r, lc) == {0: "slab", 1: "gram", 2: "cspace"}[lc]
    for form, N, C, r, chains in SC.DEFICIENT:
        for lc in chains:
            assert SC.chain_taken(N, C, r, lc) == {0: "slab", 1: "gram", 2: "cspace"}[lc], (form, N, C, r, lc)


def test_inputs_are_the_same_on_every_call():
    a, b = SC.flat(33, 136, 8, 0), SC.flat(33, 136, 8, 0)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    assert not np.array_equal(SC.flat(33, 136, 8, 1)[0], a[0])
    x, base, q0 = a
    assert x.dtype == F16 and base.dtype == F16 and q0.dtype == np.float32 and q0.shape == (136, 8)
    q = SC.flat(33, 136, 12, 0)[2]
    assert q.shape == (136, 16) and not q[:, 12:].any() and np.abs(q[:, :12].T @ q[:, :12] - np.eye(12)).max() < 1e-6
    # flat: min(N, C, 48) equal singular values well above the noise
    s = np.linalg.svd(SC.residual(*SC.flat(100, 264, 8, 0)[:2]).astype(np.float64), compute_uv=False)
    assert s[47] / s[0] > 0.9 and s[48] / s[0] < 0.05
