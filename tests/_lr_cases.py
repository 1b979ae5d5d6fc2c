"""The input domain of the low-rank RECEIVER (k_lr_decode, k_lr_decode_mfma, k_lr_dq4) as deterministic cases - a plain module in the manner
of tests/_value_cases.py, shared by tests/test_lr_f64_host.py (CPU: the witness against planted errors, every case against its `why`, the
pinned-share condition) and tests/test_gpu_lr_receiver.py (GPU: the kernels against the witness).

    CASES                                   (name, why)
    build(name, N, C, r, rep=0, quant=False) -> (U (N, r), V (r, C), base (N, C)) fp16 arrays, the same on every call
    plain_packet(U, V)                      the LOW_RANK packet [U | V] as uint16 words
    q_packet(U, V)                          the LOW_RANK_Q packet of (U, V^T) by the pinned int4 oracle, as bytes
    rows_per_wg(N, C, batch)                the host rule of cfx_i_lr_decode_launch for the MFMA form, restated

quant=True builds the variant whose factors are meant for the int4 quantiser (N even, r % 8 == 0): `integers` and `one-hot` then survive
it EXACTLY (every factor column spans a range of 15 or 0: scale fp16(15 / 15.000001) = 1 or 0), `large` leaves room for the
quantisation error; the other cases are what they are - the witness dequantises the packet itself.

Shapes: the smallest that take every branch of the kernels (see tests/test_gpu_lr_receiver.py)."""
import zlib

import numpy as np

F16, F64 = np.float16, np.float64
ULP0 = 2.0 ** -24                # fp16's smallest subnormal

RANKS = (2, 8, 12, 16, 18, 24, 32)              # RP = 8, 16, 32; r == RP and r != RP
RANKS_Q = (8, 16, 24, 32)
NS = (1, 5, 31, 33, 37)                         # a lone row; a tile whose rb = ra + 4 partner is missing; both sides of the 32-row tile
NS_Q = (2, 6, 34, 70)                           # N = 2 (mod 4) with r = 8 or 24: the V^T section starts 8 bytes off a 16-byte boundary
CS = (8, 24, 520, 1032)                         # one lane; a partial wave; one column past a 512 block; two blocks and a tail
WALK_BATCH = 16
# the multi-pass MFMA walk at batch 16: (quantised, N, C, rows a workgroup walks)  (LOW_RANK_Q needs an even N: 130 for 129, 38 for 37)
WALK = [(False, 129, 11784, 128), (False, 70, 11784, 64), (False, 37, 1032, 32),
        (True, 130, 11784, 128), (True, 70, 11784, 64), (True, 38, 1032, 32)]
WALK_RANKS = {False: (18, 32), True: (24, 32)}
WALK_CASES = ("integers", "one-hot", "random")
BATCH_SHAPE, BATCH_RANKS = (34, 520), (8, 32)   # batch 1, 3, 16 of distinct packets; the in-place call
SENDER_SHAPE = (64, 512)
TABLE_SHAPE = (200, 1024)                       # the pinned-share table of docs/DESIGN_DETAIL.md

CASES = [
    ("random", "U = randn / sqrt(r), V = randn, base = randn: the ordinary case; the witness pins at least 80 % of it"),
    ("integers", "factor entries are integers in +-8 and base entries are integers: every sum is exact in any order, the interval is one "
     "value everywhere, the comparison is bit for bit"),
    ("one-hot", "row n of U is non-zero at k = n mod r only and V[k][c] encodes (k, c) (plain: distinct within every column, and along a row "
     "for 16381 / r columns; quantised: 16 levels, k and k + 1 differ): out[n][c] is base + u V[n mod r][c] exactly, so a wrong k-lane of an "
     "MFMA fragment, a missing k0 + e < r guard or a transposed index is a wrong value, not noise"),
    ("large", "|p| up to about 6e4 (quantised: 4.5e4) with |p| + e and base + p finite"),
    ("zero-rows", "all-zero rows of U under -0 and +0 base elements"),
    ("subnormal-factors", "whole units of 2^-24 mixed into both factors"),
]
NAMES = [n for n, _ in CASES]
EXACT = ("integers", "one-hot")                 # pinned 100 %


def rows_per_wg(N, C, batch):
    """csrc/cfx_lowrank.hip cfx_i_lr_decode_launch, MFMA form: 128 or 64 rows a workgroup where that still leaves 768 workgroups"""
    cb = -(-C // 512)
    for cand in (128, 64):
        if cb * -(-N // cand) * batch >= 768:
            return cand
    return 32


def _random(rng, N, C, r, quant):
    return rng.standard_normal((N, r)) / np.sqrt(r), rng.standard_normal((r, C)), rng.standard_normal((N, C))


def _integers(rng, N, C, r, quant):
    if not quant:
        return rng.integers(-8, 9, (N, r)), rng.integers(-8, 9, (r, C)), rng.integers(-64, 65, (N, C))
    U, V = rng.integers(-8, 8, (N, r)), rng.integers(-8, 8, (r, C))          # [-8, 7] with both ends in every column of U and of V^T
    k = np.arange(r)
    U[k % N, k], U[(k + 1) % N, k] = -8, 7
    V[k, (3 * k) % C], V[k, (3 * k + 1) % C] = -8, 7
    return U, V, rng.integers(-64, 65, (N, C))


def _one_hot(rng, N, C, r, quant):
    n, k, c = np.arange(N), np.arange(r)[:, None], np.arange(C)[None, :]
    U = np.zeros((N, r))
    if not quant:
        U[n, n % r] = 1.0
        # (k, c) as fp16 BITS: element c * r + k of the 16381 values from 2^-4 up (16381 is prime: no period that r or a tile width
        # divides); distinct within a column, within a row for 16381 / r columns, and from its transposed position
        V = (np.uint16(0x2C00) + ((c * r + k) % 16381).astype(np.uint16)).view(F16).astype(F64)
    else:
        U[n, n % r] = 15.0                                               # range 15 (or 0): the quantiser's scale is 1 (or 0), the codes are exact
        V = (7 * c + 3 * k) % 16 * 1.0
        kk = np.arange(r)
        V[kk, (2 * kk) % C], V[kk, (2 * kk + 1) % C] = 0.0, 15.0
    return U, V, rng.integers(-64, 65, (N, C))


def large_target(quant):
    return 4.5e4 if quant else 6.0e4


def _large(rng, N, C, r, quant):
    t = large_target(quant)
    U = rng.choice([-1.0, -0.5, 0.5, 1.0], (N, r))
    V = np.where(rng.integers(0, 2, (r, C)) == 1, 1.0, -1.0) * (t / r) * rng.uniform(0.5, 1.0, (r, C))
    V[:, 0] = np.where(np.arange(r) % 2 == 0, 1.0, -1.0) * (t / r)      # row 0 of U lines up with column 0 of V: p[0][0] = the target
    U[0] = np.sign(V[:, 0])
    V[:, C - 1] = -V[:, 0]                                               # ... and with the last column: - the target
    return U, V, rng.standard_normal((N, C)) * 100.0


def zero_rows(N):
    return [n for n in range(N) if n % 3 == 1 or n == N - 1]


def _zero_rows(rng, N, C, r, quant):
    U, V, base = _random(rng, N, C, r, quant)
    z = zero_rows(N)
    U[z] = 0.0
    base = base.astype(F16)
    bz = np.where((np.arange(C)[None, :] + np.array(z)[:, None]) % 2 == 0, np.uint16(0x8000), np.uint16(0))
    base.view(np.uint16)[z] = bz
    return U, V, base


def _subnormal(rng, N, C, r, quant):
    U, V, base = _random(rng, N, C, r, quant)
    mu, mv = rng.integers(0, 3, (N, r)) == 0, rng.integers(0, 3, (r, C)) == 0
    U[mu] = (rng.integers(-1023, 1024, (N, r)) * ULP0)[mu]
    V[mv] = (rng.integers(-1023, 1024, (r, C)) * ULP0)[mv]
    return U, V, base


_GEN = {"random": _random, "integers": _integers, "one-hot": _one_hot, "large": _large, "zero-rows": _zero_rows, "subnormal-factors": _subnormal}


def build(name, N, C, r, rep=0, quant=False):
    rng = np.random.default_rng(zlib.crc32(f"lr-{name}-{N}-{C}-{r}-{rep}-{int(quant)}".encode()))
    U, V, base = _GEN[name](rng, N, C, r, quant)
    U, V, base = (np.ascontiguousarray(a, dtype=F16) for a in (U, V, base))
    assert U.shape == (N, r) and V.shape == (r, C) and base.shape == (N, C)
    return U, V, base


def plain_packet(U, V):
    return np.concatenate([np.ascontiguousarray(U, dtype=F16).reshape(-1), np.ascontiguousarray(V, dtype=F16).reshape(-1)]).view(np.uint16)


def q_packet(U, V):
    """[int4(U) | int4(V^T)] by oracle/ref_np.py compress("int4", M, None) - the pinned oracle tests/test_value_domain_f64.py holds to float64"""
    from oracle import ref_np as R
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        pu, _ = R.compress("int4", np.ascontiguousarray(U, dtype=F16), None)
        pv, _ = R.compress("int4", np.ascontiguousarray(np.asarray(V, dtype=F16).T), None)
    return np.concatenate([np.asarray(pu).view(np.uint8).reshape(-1), np.asarray(pv).view(np.uint8).reshape(-1)])


def packet(quant, U, V):
    """the wire packet as uint16 words (both forms are a whole number of halves)"""
    return q_packet(U, V).view(np.uint16) if quant else plain_packet(U, V)


PIN_MIN = 0.80


def factors_seen(quant, U, V):
    """the factors the receiver multiplies: LOW_RANK_Q sees them through the int4 packet"""
    if not quant:
        return U, V
    import _lr_f64_check as W
    return W.split_q(q_packet(U, V), U.shape[0], V.shape[1], U.shape[1])


def random_rep(quant, N, C, r, withbase):
    """the draw of `random` the every-instantiation test uses at a shape: the first (from 0 with a base, from 1 without) on which the
    witness alone pins PIN_MIN of the elements.  A condition on the input, known before any kernel runs: at 8 or 24 elements a draw
    can fall below it by two elements, and an interval test on it would prove little."""
    import _lr_f64_check as W
    for rep in range(0 if withbase else 1, 64):
        U, V, base = build("random", N, C, r, rep, quant)
        if W.pinned_share(*factors_seen(quant, U, V), base if withbase else None) >= PIN_MIN:
            return rep
    raise AssertionError(("no draw pins enough", quant, N, C, r, withbase))


def gpu_random_draws():
    """every `random` draw tests/test_gpu_lr_receiver.py decodes: (quant, N, C, r, rep, with base)"""
    out = []
    for quant, ns, ranks in ((False, NS, RANKS), (True, NS_Q, RANKS_Q)):
        for r in ranks:
            for N in ns:
                for C in CS:
                    out.append((quant, N, C, r, random_rep(quant, N, C, r, True), True))
                    out.append((quant, N, C, r, random_rep(quant, N, C, r, False), False))          # the batch's item without a base
    for quant, N, C, _ in WALK:                                      # item i of the walk's random batch is draw i % 4
        for r in WALK_RANKS[quant]:
            for rep in range(4):
                out.append((quant, N, C, r, rep, rep != 3))
    for quant in (False, True):                                      # batch 1, 3, 16 and the in-place call
        for r in BATCH_RANKS:
            for i in range(16):
                out.append((quant,) + BATCH_SHAPE + (r, i, True))
                out.append((quant,) + BATCH_SHAPE + (r, i, False))
    return out
