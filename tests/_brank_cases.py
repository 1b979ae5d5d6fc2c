"""The domain cfx_binary_rank_compress_batch / cfx_binary_rank_decompress_batch accept as deterministic cases - a plain module in the manner
of tests/_lr_cases.py and tests/_lr_sender_cases.py, shared by tests/test_brank_host.py (CPU: the witness of tests/_brank_witness.py
against oracle/ref_np.py and against planted errors, the visibility of a lost |.| in the factor chains, the coverage of the lists) and
tests/test_gpu_brank.py (GPU: k_binary_rank bit for bit, the |x - base| branches of the three factor chains against the float64 witness
of tests/_lr_sender_f64.py).

    KERNEL                                  (N, C, K): the shapes of k_binary_rank (R = 8 rows a tile, TILE_C = 512, factors 8 at a time)
    KINDS, build(kind, N, C, K, rep)        -> dict(x, base, U (N, K), V (C, K)) fp16: the value kinds of crafted packets
    scattered(N, C, rank, rep)              -> (x, base, q0): the sender input whose |x - base| has a flat spectrum
    deficient(form, N, C, rank)             -> (x, base, q0) with rank(|x - base|) < rank
    CSPACE, GRAM, SLAB, FALLS, DEFICIENT    the chain cases, every shape with the branch it is there for (MOVED: where the codec refuses one)
    chain_case(N, C, rank)                  -> (x, base, q0, Ref of |fp16(x - base)|), computed once

Why scattered blocks: |x - base| is non-negative, and the |.| of flat() of tests/_lr_sender_cases.py has one dominant direction (its
mean).  Positive rank-1 blocks on disjoint (row group, column group) pairs are orthogonal to each other whatever their entries: k equal
singular values, nothing converges, a product that loses a tile or a |.| that is missing on a tail moves U V by hundreds of bounds.  The
random signs make x - base itself look nothing like its |.|."""
import zlib

import numpy as np

import _lr_sender_cases as SC

F16, F32, F64 = np.float16, np.float32, np.float64
ULP0 = 2.0 ** -24

NS = (1, 2, 7, 8, 9, 17)                         # a lone row; a tile of two; one short of, at and one past R = 8; two tiles and a tail
CS = (8, 16, 24, 504, 512, 520, 1032)            # one lane; two; three; one lane short of TILE_C = 512; at it; one lane past; two blocks and a tail
KS = (1, 2, 3, 7, 8, 9, 12, 16, 17, 31, 32)      # below, at and past every chunk of 8 factors; odd and even
BATCHES = (1, 3, 16)                             # item 1 of a batch has no base


def accepted(N, C, K=1):
    return N >= 1 and C >= 8 and C % 8 == 0 and 1 <= K <= 32 and (N * (C // 8)) % 2 == 0


def c_class(C):
    return "below" if C < 512 else ("at" if C == 512 else "past")


def _kernel_shapes():
    """every accepted (N, C) pair with two ranks, dealt round so that every K meets every kind of pair: 22 pairs, 44 shapes and one more"""
    pairs = [(N, C) for N in NS for C in CS if accepted(N, C)]
    out = []
    for i, (N, C) in enumerate(pairs):
        for j in (0, 1):
            out.append((N, C, KS[(2 * i + 5 * j + i // len(KS)) % len(KS)]))
    return out + [(8, 512, 16)]          # whole tiles, whole chunks: the one pair that has both got odd ranks from the deal


KERNEL = _kernel_shapes()
REFUSED_PAIRS = [(N, C) for N in NS for C in CS if not accepted(N, C)]      # N * C / 8 odd

KINDS = [
    ("random", "U = |randn| / sqrt(K) with random signs, V = randn, base = randn, x = base + randn: the ordinary case"),
    ("integers", "factor entries are integers in +-8, base and x integers: every product and every sum is exact"),
    ("one-hot", "row n of U is non-zero at k = n mod K only and V[c, k] encodes (k, c): scale[n, c] = V[c, n mod K] exactly, so a wrong "
     "k-lane, a missing k0 + k < K guard or a transposed index is a wrong value, not noise"),
    ("large", "products of one sign per element with sums from a quarter of 7e4 up to it: scales up to the top of fp16 and past it (inf), "
     "base rows at +-6e4 so that base + recv overflows too"),
    ("subnormal", "factors in whole units of 2^-24 and factors whose products are: the fp16 product is subnormal and must be kept"),
    ("signed-zeros", "+-0 in base, x == base, x = -0 against base = +0 and the reverse; every other row of U and column of V all -0"),
    ("nan-x", "a few NaN activations (either sign bit set): their sign bit on the wire is 0, the state is base -+ scale as anywhere"),
]
KIND_NAMES = [n for n, _ in KINDS]


def _rng(*key):
    return np.random.default_rng(zlib.crc32("-".join(str(k) for k in key).encode()))


def build(kind, N, C, K, rep=0):
    """dict(x, base, U, V), fp16, read-only; the same on every call"""
    rng = _rng("brank", kind, N, C, K, rep)
    base = rng.standard_normal((N, C))
    x = base + rng.standard_normal((N, C))
    U = np.abs(rng.standard_normal((N, K))) / np.sqrt(K) * rng.choice([-1.0, 1.0], (N, K))
    V = rng.standard_normal((C, K))
    n, c, k = np.arange(N), np.arange(C)[:, None], np.arange(K)[None, :]
    if kind == "integers":
        U, V = rng.integers(-8, 9, (N, K)), rng.integers(-8, 9, (C, K))
        base = rng.integers(-64, 65, (N, C))
        x = base + rng.integers(-64, 65, (N, C))
    elif kind == "one-hot":
        U = np.zeros((N, K))
        U[n, n % K] = 1.0
        # (k, c) as fp16 BITS from 2^-4 up (16381 is prime: no period a rank or a tile width divides), as tests/_lr_cases.py does
        V = (np.uint16(0x2C00) + ((c * K + k) % 16381).astype(np.uint16)).view(F16).astype(F64)
    elif kind == "large":
        t = 7.0e4
        U = rng.choice([0.5, 1.0], (N, K))
        V = (t / K) * rng.uniform(0.5, 1.0, (C, K)) * rng.choice([-1.0, 1.0], (C, 1))      # one sign per column: no inf - inf in a sum
        U[0] = 1.0
        V[0], V[C - 1] = t / K, -t / K                                                    # the target itself, either sign: past 65504
        base = rng.standard_normal((N, C)) * 100.0
        base[N - 1] = 6.0e4 * np.where(np.arange(C) % 2 == 0, 1.0, -1.0)
        x = base + rng.standard_normal((N, C)) * 1000.0
    elif kind == "subnormal":
        mu, mv = rng.integers(0, 3, (N, K)) == 0, rng.integers(0, 3, (C, K)) == 0
        U[mu] = (rng.integers(-1023, 1024, (N, K)) * ULP0)[mu]
        V[mv] = (rng.integers(-1023, 1024, (C, K)) * ULP0)[mv]
        U[:, 0] = rng.integers(-63, 64, N) * 2.0 ** -12                                   # u v in whole units of 2^-24, below 2^-14
        V[:, 0] = rng.integers(-15, 16, C) * 2.0 ** -12
    elif kind == "signed-zeros":
        U[1::2] = -0.0
        V[1::2] = -0.0
        if N == 1:
            U[:] = -0.0
        base, x = base.astype(F16), x.astype(F16)
        m = (np.arange(N)[:, None] + np.arange(C)[None, :]) % 4
        base.view(np.uint16)[m == 0] = 0x8000                                             # -0 under any x
        x[m == 1] = base[m == 1]                                                          # x - base = +0
        base.view(np.uint16)[m == 2] = 0x0000
        x.view(np.uint16)[m == 2] = 0x8000                                                # -0 - +0 = -0: bit 1
        base.view(np.uint16)[m == 3] = np.where(np.arange(int((m == 3).sum())) % 2 == 0, 0x8000, 0x0000)
        x.view(np.uint16)[m == 3] = np.where(np.arange(int((m == 3).sum())) % 3 == 0, 0x0000, 0x8000)
    elif kind == "nan-x":
        x = x.astype(F16)
        idx = rng.choice(N * C, size=max(2, N * C // 50), replace=False)
        x.reshape(-1).view(np.uint16)[idx] = np.where(np.arange(idx.size) % 2 == 0, 0x7E00, 0xFE01)
    elif kind != "random":
        raise KeyError(kind)
    with np.errstate(over="ignore"):
        out = {k_: np.ascontiguousarray(v, dtype=F16) for k_, v in dict(x=x, base=base, U=U, V=V).items()}
    assert out["U"].shape == (N, K) and out["V"].shape == (C, K)
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- sender inputs for the factor chains --------------------------------------------------------------------------------------------------
def scattered(N, C, rank, rep=0):
    """x, base (fp16), q0 (fp32 (C, lr_rank_pad(rank))): |fp16(x - base)| has k = min(N, C, 48) equal singular values"""
    rng = _rng("brank-scattered", N, C, rank, rep)
    k = min(N, C, 48)
    rows, cols = np.array_split(rng.permutation(N), k), np.array_split(rng.permutation(C), k)
    M = np.zeros((N, C))
    for g in range(k):
        u, v = rng.uniform(0.5, 1.5, rows[g].size), rng.uniform(0.5, 1.5, cols[g].size)
        M[np.ix_(rows[g], cols[g])] = np.outer(u, v) / (np.linalg.norm(u) * np.linalg.norm(v))
    M = M * 0.05 * np.sqrt(N * C) + 1e-3 * np.abs(rng.standard_normal((N, C)))
    S = rng.choice([-1.0, 1.0], (N, C))
    base = rng.standard_normal((N, C)).astype(F16)
    x = (base.astype(F32) + (S * M).astype(F32)).astype(F16)
    return x, base, SC._q0(rng, C, rank)


def deficient(form, N, C, rank):
    """"abs-rank1": x - base = +-c, exact in fp16: |A| has rank 1 exactly while A has full rank; "zero": x == base; "short": rank > min(N, C)"""
    rng = _rng("brank-deficient", form, N, C, rank)
    if form == "short":
        assert rank > min(N, C)
        x, base, _ = scattered(N, C, 1)
        return x, base, SC._q0(rng, C, rank)
    base = rng.integers(-8, 9, (N, C)).astype(F16)
    if form == "zero":
        return base.copy(), base, SC._q0(rng, C, rank)
    assert form == "abs-rank1" and rank > 1
    D = rng.choice([-0.375, 0.375], (N, C))
    x = (base.astype(F64) + D).astype(F16)
    assert np.array_equal(x.astype(F64), base.astype(F64) + D) and np.linalg.matrix_rank(D) == min(N, C)
    return x, base, SC._q0(rng, C, rank)


def abs_residual(x, base):
    """|fp16(x - base)|: the matrix the chains factorise"""
    return np.abs(SC.residual(x, base))


# C-space chain (k_lr_aq<RP, true, false> forms |x - base|): cfx_set_lr_chain(ctx, 2)
# (an odd N needs an even C / 8 - the sign-bit section is N C / 8 bytes and the fp16 factors follow it: (5, 8), (31, 24), (33, 136) and
# (33, 520) are refused by cfx_binary_rank_packet_bytes, see MOVED; their rows stay, their column tail is 16 columns instead of 8.  The
# 8-column tails are those of the even N: 264, 520, 1032, 136)
CSPACE = [
    (5, 16, 3, "N < 32 and C < 32: one partial row tile, one partial 32-column tile; odd rank at RP = 8"),
    (31, 16, 7, "one row short of a tile; C = 16; odd rank one below RP = 8: factor rows of stride 7"),
    (33, 144, 9, "one row past a tile; a column tail past 128; the first odd rank at RP = 16"),
    (100, 264, 17, "four row tiles, the last of 4 rows; a tail past 256; the first odd rank at RP = 32: k_lr_apply2 between the products"),
    (100, 1032, 31, "five column chunks over four groups; the last odd rank"),
    (100, 520, 8, "r == RP = 8 (the fused product); three chunks, group 3 owns none"),
    (600, 136, 5, "two row splits of k_lr_aty: 384 + 216 rows"),
    (33, 528, 32, "r == RP = 32; a column tail past 512"),
    (64, 256, 12, "even rank at RP = 16; a shape the N-space chains take unless forced"),
]
# Gram six-launch chain (k_lrg_prep forms |x - base|): cfx_set_lr_chain(ctx, 1), RP <= 16
GRAM = [
    (32, 128, 1, "one 32-row tile, half of NP = 64 is padding; rank 1: factor rows of stride 1"),
    (65, 256, 5, "one row past a 64-row tile; odd rank at RP = 8"),
    (129, 512, 13, "six tile pairs, KS = 8; odd rank at RP = 16"),
    (100, 384, 16, "r == RP = 16; KS = 2"),
    (576, 640, 9, "the tallest the chain takes, kslab 320; odd rank at RP = 16"),
    (100, 128, 8, "r == RP = 8: the even rank at RP = 8"),
]
# slab-resident chain (k_lrs forms |x - base| in its first phase): chain 0 on the default stream
SLAB = [
    (32, 512, 3, "one 32-row tile; odd rank at RP = 8"),
    (33, 640, 1, "one row past a tile, 20 slabs; rank 1"),
    (100, 512, 12, "even rank, r != RP = 16"),
    (100, 640, 31, "odd rank at RP = 32: the blocked factorisation"),
    (576, 512, 17, "the tallest; the first odd rank at RP = 32"),
    (576, 640, 32, "r == RP = 32 at 576 rows"),
    (100, 512, 8, "r == RP = 8: the even rank at RP = 8"),
    (65, 640, 13, "odd rank at RP = 16"),
]
# a rank-32 call under chain 1 falls to the C-space chain (the Gram chain is built for RP <= 16)
FALLS = [(100, 512, 32, "rank 32 under chain 1: C-space")]
# (form, N, C, rank, chains it runs on)
DEFICIENT = [
    ("abs-rank1", 33, 144, 5, (2,)),
    ("abs-rank1", 100, 512, 9, (0, 1, 2)),
    ("abs-rank1", 100, 512, 32, (0, 2)),
    ("zero", 33, 144, 3, (2,)),
    ("zero", 100, 512, 7, (0, 1, 2)),
    ("short", 5, 16, 7, (2,)),
    ("short", 20, 520, 31, (2,)),
]
# batches of distinct tensors, item 1 without a base: (lr_chain, N, C, rank)
BATCH_SHAPES = [(2, 33, 144, 9), (1, 65, 256, 5), (0, 100, 512, 12)]
# the Python paths' awkward shape
PY_SHAPE = (9, 520, 3)                          # refused for the same reason: the Python paths say so, and run at (10, 520, 3)

# shapes one would list for the C-space chain that the codec refuses (N C / 8 odd) -> the listed shape that stands in
MOVED = {(5, 8, 3): (5, 16, 3), (31, 24, 7): (31, 16, 7), (33, 136, 9): (33, 144, 9), (33, 520, 32): (33, 528, 32)}
CHAIN_NAME = {0: "slab", 1: "gram", 2: "cspace"}
# the draw of scattered() a (N, C, rank) uses where draw 0 does not let every planted fault move the projection by 4 x its bound
REPS = {}
# shapes that cannot meet the condition for one fault, with the reason (at most one listed case in ten)
DROPPED = {}


def rep_of(N, C, rank):
    return REPS.get((N, C, rank), 0)


def all_chain_cases():
    """(chain name, lr_chain, N, C, rank, why)"""
    return [("cspace", 2) + c for c in CSPACE] + [("gram", 1) + c for c in GRAM] + [("slab", 0) + c for c in SLAB] \
        + [("cspace", 1) + c for c in FALLS]


_refs = {}


def chain_case(N, C, rank, rep=None):
    """-> (x, base, q0, Ref(|fp16(x - base)|, q0, rank, "flat")): one reference per case, shared by every test, never written to"""
    import _lr_sender_f64 as W
    rep = rep_of(N, C, rank) if rep is None else rep
    k = (N, C, rank, rep)
    if k not in _refs:
        x, base, q0 = scattered(N, C, rank, rep)
        for a in (x, base, q0):
            a.setflags(write=False)
        _refs[k] = (x, base, q0, W.Ref(abs_residual(x, base), q0, rank, "flat"))
    return _refs[k]


def deficient_case(form, N, C, rank):
    import _lr_sender_f64 as W
    k = (form, N, C, rank)
    if k not in _refs:
        x, base, q0 = deficient(form, N, C, rank)
        for a in (x, base, q0):
            a.setflags(write=False)
        _refs[k] = (x, base, q0, W.Ref(abs_residual(x, base), q0, rank, "deficient"))
    return _refs[k]


# ---- planted faults of the |.| branches: the replay runs on a matrix whose |.| is missing somewhere, or loses part of a product ---------
def last_tile_rows(N):
    """rows of the last 32-row tile of k_lr_aq / k_lrg_prep / k_lrs"""
    return N - (N - 1) // 32 * 32


ABS_FAULTS = ("|.| dropped on the column tail chunk", "|.| dropped on the last row tile", "|.| dropped on the second row split",
              "a row tile dropped from a product", "a column chunk dropped from a product")


def planted(name, x, base, N, C):
    """-> (matrix the faulty chain factorises, fault for W.replay) or None where the shape has no such branch"""
    import _lr_sender_f64 as W
    A = SC.residual(x, base).astype(F64)
    B = np.abs(A)
    ident = lambda nm, M, c: M
    if name == "|.| dropped on the column tail chunk":                      # the last 8 columns: the width of one lane's load
        B[:, C - 8:] = A[:, C - 8:]
        return B, ident
    if name == "|.| dropped on the last row tile":
        n0 = N - last_tile_rows(N)
        B[n0:] = A[n0:]
        return B, ident
    if name == "|.| dropped on the second row split":
        ns, rps, nz = SC.aty_splits(N, C)
        if nz < 2:
            return None
        B[rps:2 * rps] = A[rps:2 * rps]
        return B, ident
    if name == "a row tile dropped from a product":                         # Z1 = A^T Y1 without the last 32-row tile
        n0 = N - last_tile_rows(N)
        if n0 <= 0:
            return None
        return B, (lambda nm, M, c: c["A"][:n0].T @ c["Y"][:n0] if nm == "Z1" else M)
    if name == "a column chunk dropped from a product":                     # Y1 = A Q1 without its last partial 32-column tile
        c0 = C - W.fault_cols(C)
        if c0 <= 0:
            return None
        return B, (lambda nm, M, c: c["A"][:, :c0] @ c["Q"][:c0] if nm == "Y1" else M)
    raise KeyError(name)
