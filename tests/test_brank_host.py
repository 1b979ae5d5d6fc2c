"""The witness of the 1-bit codec with rank-K scales (tests/_brank_witness.py) and its cases (tests/_brank_cases.py) on the CPU:

  * the witness against oracle/ref_np.py binary_rank_apply / unpack_bits_1 / pack_bits_1 on every kernel shape and value kind - two
    independent statements of one contract, bit for bit - and against every planted error of a kernel (FAULTS);
  * every value kind is what its `why` says;
  * every chain case: the float32 port of the reference iteration on |x - base| meets the float64 contract of tests/_lr_sender_f64.py, and
    a chain that loses the |.| on a tail, or a tile of a product, moves the projection by at least 4 x the case's own bound;
  * the case lists cover what they claim; cfx_binary_rank_packet_bytes / _workspace_bytes over the whole small domain."""
import numpy as np
import pytest

import _brank_cases as BC
import _brank_witness as BW
import _lr_sender_cases as SC
import _lr_sender_f64 as W
from oracle import ref_np as R

F16 = np.float16
SEPARATION = 4.0
CHAINS = BC.all_chain_cases()


# ---- 1. the witness of k_binary_rank --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", BC.KIND_NAMES)
def test_witness_is_the_oracle_bit_for_bit(kind):
    for N, C, K in BC.KERNEL:
        v = BC.build(kind, N, C, K)
        for base in (v["base"], None):
            bits = BW.sign_bits(v["x"], base)
            d = v["x"] if base is None else (v["x"] - base).astype(F16)
            assert np.array_equal(bits, R.pack_bits_1(d)), (kind, N, C, K)
            assert np.array_equal(BW.unpack(bits, C), R.unpack_bits_1(bits).astype(bool))
            mine = BW.apply(bits, v["U"], v["V"], base)
            want = R.binary_rank_apply(base, R.unpack_bits_1(bits), v["U"], v["V"])
            assert BW.same(mine, want), (kind, N, C, K, base is None, BW.differing(mine, want))
            pk, nb = BW.sender(v["x"], base, v["U"], v["V"])
            b2, U2, V2 = BW.split(pk, N, C, K)
            assert pk.size == BW.packet_bytes(N, C, K) and np.array_equal(b2, bits)
            assert np.array_equal(U2.view(np.uint16), v["U"].view(np.uint16)) and np.array_equal(V2.view(np.uint16), v["V"].view(np.uint16))
            assert BW.same(nb, mine)
            assert np.array_equal(BW.sender(v["x"], base, v["U"], v["V"], ef=False)[1].view(np.uint16), v["x"].view(np.uint16))


APPLIES = {"chunk dropped": lambda N, C, K: K > 8, "no k guard": lambda N, C, K: K % 8 != 0 and N > 1,
           # (K = 1: the rounded product is the scale either way; K = 2: the fp32 sum of two fp16 values is exact, so both round once)
           "product not rounded": lambda N, C, K: K >= 2, "fp16 sum": lambda N, C, K: K >= 3, "V as (K, C)": lambda N, C, K: K >= 2}


@pytest.mark.parametrize("fault", BW.FAULTS)
def test_witness_rejects_planted_errors(fault):
    """on `random` every shape with at least 64 elements the error can touch shows it; `one-hot` shows the index errors as wrong values"""
    seen = {}
    for N, C, K in BC.KERNEL:
        if not APPLIES[fault](N, C, K):
            continue
        for kind in ("random", "one-hot", "integers"):
            v = BC.build(kind, N, C, K)
            bits = BW.sign_bits(v["x"], v["base"])
            bad = BW.differing(BW.apply(bits, v["U"], v["V"], v["base"]), BW.apply(bits, v["U"], v["V"], v["base"], fault))
            seen[(kind, N, C, K)] = bad
    rnd = {k: n for k, n in seen.items() if k[0] == "random" and k[1] * k[2] >= 64}
    assert rnd and all(rnd.values()), {k: n for k, n in rnd.items() if not n}
    assert {k[3] for k in rnd} == {K for _, _, K in BC.KERNEL if APPLIES[fault](2, 8, K)}, "every rank the error applies to"
    if fault in ("chunk dropped", "V as (K, C)"):
        hot = {k: n for k, n in seen.items() if k[0] == "one-hot" and k[1] > (8 if fault == "chunk dropped" else 1)}
        assert hot and all(hot.values()), {k: n for k, n in hot.items() if not n}
    if fault in ("chunk dropped", "no k guard", "V as (K, C)"):          # exact sums: nothing but a wrong operand changes them
        assert any(n for k, n in seen.items() if k[0] == "integers")
    if fault in ("product not rounded", "fp16 sum"):
        assert not any(n for k, n in seen.items() if k[0] in ("integers", "one-hot")), "exact cases cannot see a rounding"


def test_value_kinds_are_what_they_say():
    for N, C, K in BC.KERNEL:
        v = {k: BC.build(k, N, C, K) for k in BC.KIND_NAMES}
        again = BC.build("random", N, C, K)
        assert all(np.array_equal(v["random"][n].view(np.uint16), again[n].view(np.uint16)) for n in again)
        # integers: the fp16 sum in any order is the exact one
        i = v["integers"]
        exact = i["U"].astype(np.float64) @ i["V"].astype(np.float64).T
        assert np.array_equal(BW.scale(i["U"], i["V"]).astype(np.float64), exact) and np.array_equal(BW.scale(i["U"], i["V"], "fp16 sum").astype(np.float64), exact)
        # one-hot: the scale is one entry of V
        h = v["one-hot"]
        assert np.array_equal(BW.scale(h["U"], h["V"]).view(np.uint16), h["V"][:, np.arange(N) % K].T.view(np.uint16))
        # large: inf among the scales, finite ones too, no NaN; base + recv overflows somewhere
        l = v["large"]
        sc = BW.scale(l["U"], l["V"])
        out = BW.apply(BW.sign_bits(l["x"], l["base"]), l["U"], l["V"], l["base"])
        assert np.isinf(sc).any() and not np.isnan(sc).any() and not np.isnan(out).any()
        assert (np.isinf(out) & np.isfinite(sc)).any() or N * C < 64, (N, C, K)
        # subnormal: subnormal factors and subnormal products that a flush would lose
        s = v["subnormal"]
        sub = lambda a: (np.abs(a) < 2.0 ** -14) & (a != 0)
        p0 = (s["U"][:, :1].astype(np.float64) * s["V"][:, :1].astype(np.float64).T).astype(F16)
        assert sub(p0).any(), (N, C, K)
        assert K < 3 or N * K < 16 or (sub(s["U"]).any() and sub(s["V"]).any()), (N, C, K)
        # signed zeros: both zeros in base and in the residual, -0 factors
        z = v["signed-zeros"]
        d = BW.residual(z["x"], z["base"])
        for a in (z["base"], d):
            assert (a.view(np.uint16) == 0x8000).any() and (a.view(np.uint16) == 0).any(), (N, C, K)
        assert (z["U"].view(np.uint16) == 0x8000).any() and (z["V"].view(np.uint16) == 0x8000).any()
        assert BW.unpack(BW.sign_bits(z["x"], z["base"]), C)[d == 0].all(), "-0 and +0 give bit 1"
        # nan-x: bit 0 at every NaN, either sign
        x = v["nan-x"]["x"]
        nan = np.isnan(x)
        assert nan.sum() >= 2 and not BW.unpack(BW.sign_bits(x, v["nan-x"]["base"]), C)[nan].any()
        assert not BW.unpack(BW.sign_bits(x, None), C)[nan].any()
        assert {int(b) >> 15 for b in x.view(np.uint16)[nan]} == {0, 1}


def test_kernel_shapes_cover_the_tile_rules():
    ks = BC.KERNEL
    assert all(BC.accepted(*s) for s in ks) and len(set(ks)) == len(ks)
    for vals, col in ((BC.NS, 0), (BC.CS, 1), (BC.KS, 2)):
        for v in vals:
            assert sum(1 for s in ks if s[col] == v) >= 2, (col, v)
    combos = {(N % 8 != 0, BC.c_class(C), K % 8 == 0) for N, C, K in ks}
    assert len(combos) == 12, combos
    assert {(N, C) for N, C, _ in ks} == {(N, C) for N in BC.NS for C in BC.CS if BC.accepted(N, C)}
    assert BC.REFUSED_PAIRS and all((N * C // 8) % 2 for N, C in BC.REFUSED_PAIRS) and (1, 8) in BC.REFUSED_PAIRS
    assert {K for _, _, K in ks if K % 2} >= {3, 7, 9, 17, 31}


# ---- 2. the chain cases -------------------------------------------------------------------------------------------------------------------
def _id(c):
    return "-".join(str(v) for v in c[:5])


@pytest.mark.parametrize("case", CHAINS, ids=_id)
def test_chain_case_accepts_the_port_and_shows_a_lost_abs(case):
    chain, lc, N, C, r, why = case
    assert SC.chain_taken(N, C, r, lc) == chain, why
    x, base, q0, ref = BC.chain_case(N, C, r)
    A = SC.residual(x, base).astype(np.float64)
    assert (ref.A >= 0).all() and np.array_equal(ref.A, np.abs(A)) and (A < 0).mean() > 0.3
    s = np.linalg.svd(ref.A, compute_uv=False)
    k = min(N, C, 48)
    assert s[0] / s[k - 1] < 1.1 and (k == min(N, C) or s[k] / s[0] < 0.05), "k equal singular values above the noise"
    Up, Vp = W._port(ref.A, q0, r)
    m = W.check(ref, Up.astype(F16), Vp.astype(F16), f"float32 port {N, C, r}")
    assert ref.proj_bound()[0] < 1.5e-3 and ref.port[0] < 1e-5, (ref.floor, ref.port)
    seps = {}
    for name in BC.ABS_FAULTS:
        p = BC.planted(name, x, base, N, C)
        if p is None:                                     # one row tile, one row split
            continue
        U, V = W.replay(p[0], q0[:, :r], fault=p[1])
        mf = W.measure(ref, U.astype(F16), V.astype(F16))
        seps[name] = mf["proj"][0] / mf["proj"][1]
    print(f"{chain} {N, C, r}: floor {ref.floor[0]:.2e} port {ref.port[0]:.2e} bound {ref.proj_bound()[0]:.2e} port/bound "
          f"{max(W.ratios(m).values()):.2f} faults x bound " + ", ".join(f"{k_}: {v:.1f}" for k_, v in seps.items()))
    assert len(seps) >= (2 if N <= 32 and C <= 32 else 3)          # (one row tile and one column tile: no product loses a whole one)
    drop = BC.DROPPED.get((N, C, r), ())
    bad = {k_: v for k_, v in seps.items() if v < SEPARATION and k_ not in drop}
    assert not bad, bad


def test_few_shapes_are_dropped():
    listed = {(N, C, r) for _, _, N, C, r, _ in CHAINS}
    assert set(BC.DROPPED) <= listed and 10 * len(BC.DROPPED) <= len(listed) and set(BC.REPS) <= listed


def test_chain_lists_cover_what_they_claim():
    by = {}
    for chain, lc, N, C, r, why in CHAINS:
        by.setdefault(chain, []).append((N, C, r, lc))
    assert set(by) == {"cspace", "gram", "slab"}
    want_rp = {"cspace": {8, 16, 32}, "gram": {8, 16}, "slab": {8, 16, 32}}
    for chain, cs in by.items():
        got = {(SC.lr_rank_pad(r), r % 2) for _, _, r, _ in cs}
        assert got == {(rp, odd) for rp in want_rp[chain] for odd in (0, 1)}, (chain, got)
    issue = {"cspace": [(5, 8, 3), (31, 24, 7), (33, 136, 9), (100, 264, 17), (100, 1032, 31), (100, 520, 8), (600, 136, 5), (33, 520, 32)],
             "gram": [(32, 128, 1), (65, 256, 5), (129, 512, 13), (100, 384, 16), (576, 640, 9)],
             "slab": [(32, 512, 3), (33, 640, 1), (100, 512, 12), (100, 640, 31), (576, 512, 17), (576, 640, 32)]}
    for chain, shapes in issue.items():
        assert {BC.MOVED.get(c, c) for c in shapes} <= {c[:3] for c in by[chain]}
    for (N, C, r), (N2, C2, r2) in BC.MOVED.items():       # moved only where the codec refuses the shape, and then only in C: same rows, same rank, same side of 32 / 128 / 512
        assert not BC.accepted(N, C, r) and BC.accepted(N2, C2, r2) and (N2, r2) == (N, r) and C2 - C in (8, -8)
        assert (C < 32) == (C2 < 32) and C // 128 == C2 // 128 and C2 % 128 != 0
    assert all(BC.accepted(N, C, r) for _, _, N, C, r, _ in CHAINS) and all(BC.accepted(N, C, r) for _, N, C, r, _ in BC.DEFICIENT)
    assert all(BC.accepted(N, C, r) for _, N, C, r in BC.BATCH_SHAPES)
    assert SC.aty_splits(600, 136)[2] == 2 and any(lc == 1 and r == 32 for _, _, r, lc in by["cspace"])
    assert {N < 32 for N, _, _, _ in by["cspace"]} == {True, False} and any(C % 128 for _, C, _, _ in by["cspace"])
    for form, N, C, r, chains in BC.DEFICIENT:
        for lc in chains:
            assert SC.chain_taken(N, C, r, lc) == BC.CHAIN_NAME[lc]
    assert {f for f, *_ in BC.DEFICIENT} == {"abs-rank1", "zero", "short"}
    assert {SC.chain_taken(N, C, r, lc) for lc, N, C, r in BC.BATCH_SHAPES} == {"cspace", "gram", "slab"}
    assert all(SC.chain_taken(N, C, r, lc) == BC.CHAIN_NAME[lc] for lc, N, C, r in BC.BATCH_SHAPES)
    assert BC.BATCHES == (1, 3, 16) and {bool(SC.xcd_group(b)) for b in BC.BATCHES} == {True, False}


@pytest.mark.parametrize("form,N,C,r,chains", BC.DEFICIENT)
def test_deficient_cases_are_deficient(form, N, C, r, chains):
    x, base, q0, ref = BC.deficient_case(form, N, C, r)
    A = SC.residual(x, base).astype(np.float64)
    assert ref.rankA < r
    if form == "abs-rank1":
        assert ref.rankA == 1 and np.linalg.matrix_rank(A) == min(N, C)
    if form == "zero":
        assert ref.rankA == 0 and not A.any()
    k = ref.rankA
    U, V = np.zeros((N, r)), np.zeros((r, C))
    if k:
        U[:, :k], V[:k] = ref.Ur, ref.Vr
    W.check(ref, U.astype(F16), V.astype(F16), f"svd factors {form, N, C, r}")
    if k:
        assert W.failures(W.measure(ref, np.zeros((N, r), F16), np.zeros((r, C), F16)))
    if k and r <= min(N, C):
        # the factors of x - base instead of |x - base|: what a chain without its |.| sends
        Ua, Va = W.replay(A, q0[:, :r])
        assert W.failures(W.measure(ref, Ua.astype(F16), Va.astype(F16)))


# ---- 3. the host's size functions -----------------------------------------------------------------------------------------------------------
def test_size_functions_over_the_small_domain():
    from compactfusion_amd import _lib
    lib = _lib.load()
    n_ok = 0
    for N in (-1, 0, 1, 2, 3, 4, 7, 8, 9, 17, 100):
        for C in (-8, 0, 4, 8, 12, 16, 24, 136, 504, 512, 520, 1032):
            for K in (-1, 0, 1, 2, 3, 8, 9, 31, 32, 33):
                want = BW.packet_bytes(N, C, K)
                assert lib.cfx_binary_rank_packet_bytes(N, C, K) == want, (N, C, K)
                assert (want != 0) == (BC.accepted(N, C, K) if N >= 1 and C >= 8 else False)
                n_ok += want != 0
                for B in (0, 1, 3, 16, 17):
                    ws = lib.cfx_binary_rank_workspace_bytes(N, C, K, B)
                    if want == 0 or not 1 <= B <= 16:
                        assert ws == 0, (N, C, K, B)
                    else:
                        one = lib.cfx_binary_rank_workspace_bytes(N, C, K, 1)
                        # per tensor: at least D (fp16), the padded fp16 factors and the start matrix; the same for every item of a batch
                        RP = SC.lr_rank_pad(K)
                        assert ws == B * one and one >= 2 * N * C + 2 * (N + C) * RP + 4 * C * RP, (N, C, K, B, ws)
                        if K % 2 == 0:
                            assert one == lib.cfx_lr_workspace_bytes(1 if K % 8 == 0 and N % 2 == 0 else 0, N, C, K, 1)
    assert n_ok > 250
    for N, C, K in BC.KERNEL:
        assert lib.cfx_binary_rank_packet_bytes(N, C, K) == N * C // 8 + 2 * (N + C) * K
    for N, C in BC.REFUSED_PAIRS:
        assert lib.cfx_binary_rank_packet_bytes(N, C, 4) == 0 and lib.cfx_binary_rank_workspace_bytes(N, C, 4, 1) == 0
