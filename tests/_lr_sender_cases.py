"""The input domain of the low-rank SENDER's factor chains as deterministic cases - a plain module in the manner of tests/_lr_cases.py,
shared by tests/test_lr_sender_f64_host.py (CPU: the witness of tests/_lr_sender_f64.py against the float32 port and against planted
faults, the coverage of the host's dispatch) and tests/test_gpu_lr_sender.py (GPU: the three chains against the witness).

    flat(N, C, rank, rep)                   -> (x, base, q0): a residual with a FLAT spectrum over min(N, C, 48) directions
    graded(N, C, rank, seed, decay, ...)    -> the decaying-spectrum input of tests/test_gpu_lowrank_slab.py (torch tensors, CPU)
    deficient(form, N, C, rank, rep)        -> (x, base, q0) with rank(x - base) < rank
    chain_taken / aty_splits / gy / lrg_ks / xcd_group     the host's dispatch rules, restated
    CSPACE, GRAM, SLAB, DEFICIENT, QUANT    the case lists, every shape with the branch it is there for

Why flat: subspace iteration corrects itself on a decaying spectrum - a wrong intermediate product barely moves U V.  With equal
singular values over more directions than the rank nothing converges: the iterated subspace is set by Q0 and by every product on the way,
and a product that loses a row split or a column tail moves U V by 1e-2 .. 3e-1 (tests/test_lr_sender_f64_host.py redoes the table)."""
import zlib

import numpy as np

F16, F32, F64 = np.float16, np.float32, np.float64


def lr_rank_pad(rank):
    return 8 if rank <= 8 else (16 if rank <= 16 else 32)


def _rng(*key):
    return np.random.default_rng(zlib.crc32("-".join(str(k) for k in key).encode()))


def _orth(rng, n, k):
    return np.linalg.qr(rng.standard_normal((n, k)))[0]


def _q0(rng, C, rank):
    q0 = np.zeros((C, lr_rank_pad(rank)), dtype=F32)
    q0[:, :rank] = _orth(rng, C, rank)
    return q0


def flat(N, C, rank, rep=0):
    """x, base (fp16) and q0 (fp32, (C, lr_rank_pad(rank)), orthonormal leading columns): x = fp16(base + D),
    D = L diag(1 .. 1) R^T over k = min(N, C, 48) orthonormal directions plus 1e-3 noise, scaled as make() of test_gpu_lowrank_slab.py"""
    rng = _rng("lrs-flat", N, C, rank, rep)
    k = min(N, C, 48)
    D = _orth(rng, N, k) @ _orth(rng, C, k).T * (N * C) ** 0.5 * 0.05 + 1e-3 * rng.standard_normal((N, C))
    base = rng.standard_normal((N, C)).astype(F16)
    x = (base.astype(F32) + D.astype(F32)).astype(F16)
    return x, base, _q0(rng, C, rank)


def graded(N, C, rank, seed, decay=0.7, resid_rank=None):
    """x, base with a residual of decaying spectrum (sigma_k = decay^k) over `resid_rank` directions (default min(N, 48)) plus a
    little noise, and the start matrix - torch tensors on the CPU, the draw tests/test_gpu_lowrank_slab.py has always used"""
    import torch
    g = torch.Generator().manual_seed(seed)
    k = resid_rank or min(N, 48)
    L = torch.linalg.qr(torch.randn(N, k, generator=g))[0]
    R = torch.linalg.qr(torch.randn(C, k, generator=g))[0]
    s = decay ** torch.arange(k, dtype=torch.float32)
    D = (L * s) @ R.t() * (N * C) ** 0.5 * 0.05
    if resid_rank is None:
        D = D + 1e-3 * torch.randn(N, C, generator=g)
    base = torch.randn(N, C, generator=g).half()
    x = (base.float() + D).half()
    q0 = torch.zeros(C, lr_rank_pad(rank))
    q0[:, :rank] = torch.linalg.qr(torch.randn(C, rank, generator=g))[0]
    return x, base, q0


def graded_np(N, C, rank, seed, decay=None):
    """graded() as numpy arrays; the decay test_projection_and_states uses: 0.7^k up to rank 16, 0.85^k above"""
    x, base, q0 = graded(N, C, rank, seed, decay=(0.7 if rank <= 16 else 0.85) if decay is None else decay)
    return x.numpy(), base.numpy(), q0.numpy()


def deficient(form, N, C, rank, rep=0):
    """rank(x - base) < rank.
    "rank3": x - base = L R^T / 64 with 3 columns of small integers and an integer base: every fp16 value and the subtraction are EXACT,
             so the residual the kernels form has rank 3 to the last bit (a real-valued one would be of full rank after x's rounding);
    "short": rank > min(N, C) - any residual will do, flat()'s is taken;
    "zero":  x == base."""
    rng = _rng("lrs-deficient", form, N, C, rank, rep)
    if form == "short":
        assert rank > min(N, C)
        x, base, _ = flat(N, C, 2, rep)
        return x, base, _q0(rng, C, rank)
    base = rng.integers(-8, 9, (N, C)).astype(F16)
    if form == "zero":
        return base.copy(), base, _q0(rng, C, rank)
    assert form == "rank3" and rank > 3 and min(N, C) > 3
    D = rng.integers(-3, 4, (N, 3)) @ rng.integers(-3, 4, (3, C)) / 64.0     # |D| <= 27 / 64 in units of 2^-6; base + D in units of 2^-6 below 16
    x = (base.astype(F64) + D).astype(F16)
    assert np.array_equal(x.astype(F64), base.astype(F64) + D) and np.linalg.matrix_rank(D) == 3
    return x, base, _q0(rng, C, rank)


def residual(x, base):
    """A = fp16(x - base): one rounding, as the kernels form it"""
    if base is None:
        return np.asarray(x, dtype=F16)
    return (np.asarray(x, dtype=F16).astype(F32) - np.asarray(base, dtype=F16).astype(F32)).astype(F16)


# ---- the host's rules, restated (whoever changes one re-derives the shapes below) ----------------------------------------------------
CUS = 256                                            # the compute units of an MI355X: what the default stream may use


def lrg_ok(N, C):
    """csrc/cfx_lrgram.hip cfx_i_lrg_ok"""
    return 32 <= N <= 576 and C % 128 == 0 and C >= 128


def lrs_ok(N, C, RP):
    """csrc/cfx_lrslab.hip cfx_i_lrs_ok without its LDS term (16 * LRS_NW * LRS_TQ = 640 rows; the LDS allows what SLAB lists)"""
    return 32 <= N <= 640 and C % 128 == 0 and C >= 512 and RP <= 32


def lrs_fit(N, C, RP, cus=CUS):
    """cfx_i_lrs_fit: tensors of a batch one slab-resident launch takes, C / 32 workgroups each, all co-resident"""
    return min(16, (cus - 2) // (C // 32)) if lrs_ok(N, C, RP) else 0


def chain_taken(N, C, rank, lr_chain=0, cus=CUS):
    """"slab", "gram" or "cspace": cfx_lr_compress_batch (csrc/cfx_lowrank.hip) and cfx_i_lrg_factors (csrc/cfx_lrgram.hip)"""
    RP = lr_rank_pad(rank)
    fit = lrs_fit(N, C, RP, cus)
    slab32 = RP == 32 and lr_chain == 0 and fit >= 1
    if not (lrg_ok(N, C) and (RP <= 16 or slab32) and lr_chain != 2):
        return "cspace"
    return "slab" if lr_chain == 0 and fit >= 1 else "gram"


def aty_splits(N, C):
    """(row splits lr_aty_splits asks for, rows per split, splits k_lr_aty is launched with): rows per split are whole 128-row chunks,
    so fewer splits than asked for can cover N"""
    tiles = -(-C // 32) * 2
    ns = max(1, min(-(-768 // tiles), 8, N // 256))
    per = -(-N // ns)
    rps = -(-per // 128) * 128
    return ns, rps, -(-N // rps)


def gy(N):
    """(gy_, gy0_): the column groups of k_lr_aq's products, of the first product"""
    rt = -(-N // 32) * 2
    g = 1 if rt >= 256 else (2 if rt >= 128 else 4)
    return g, min(4, 2 * g)


def lrg_ks(C):
    return 8 if C % 512 == 0 else (4 if C % 256 == 0 else 2)


def xcd_group(batch):
    """the Gram chain keeps a tensor's workgroups on its own XCDs when the batch divides 8 (0: tensor after tensor)"""
    return 8 // batch if batch <= 8 and 8 % batch == 0 else 0


# ---- the cases: (N, C, rank, branch) ------------------------------------------------------------------------------------------------------
# C-space chain (k_lr_aq, k_lr_aty, k_lr_apply2): forced with cfx_set_lr_chain(ctx, 2); the shapes cfx_i_lrg_ok refuses take it under 0 too
CSPACE = [
    (5, 8, 2, "N < 32 and C < 32: one partial row tile, one partial 32-column tile; three of four column groups own no chunk"),
    (5, 136, 2, "N < 32; a column tail past 128"),
    (5, 1032, 2, "N < 32; column group 0 owns a second chunk of 8 columns"),
    (31, 24, 8, "one row short of a tile; a partial 32-column tile; r == RP = 8 (fused ORTH product)"),
    (31, 136, 12, "r != RP = 16"),
    (31, 264, 16, "a tail past 256: a second chunk of 8 columns for group 1; r == RP = 16"),
    (31, 520, 18, "RP = 32 with r != RP: k_lr_apply2 between the products"),
    (31, 1032, 24, "five chunks over four groups; RP = 32"),
    (33, 8, 2, "one row past a tile; C = 8"),
    (33, 24, 12, "C = 24, RP = 16"),
    (33, 136, 8, "two row tiles, the second of one row"),
    (33, 264, 24, "RP = 32, r != RP"),
    (33, 520, 32, "r == RP = 32"),
    (33, 1032, 16, "RP = 16 over five chunks"),
    (100, 8, 2, "four row tiles, the last of 4 rows; C = 8"),
    (100, 24, 2, "r = 2 with room to spare"),
    (100, 24, 16, "C = 24 with RP = 16: Q's tile is mostly padding"),
    (100, 136, 32, "r == RP = 32"),
    (100, 264, 18, "RP = 32, r != RP"),
    (100, 520, 8, "three chunks: group 3 owns none"),
    (100, 1032, 12, "r != RP = 16"),
    (100, 1032, 32, "r == RP = 32 over five chunks"),
    (600, 136, 8, "two row splits of k_lr_aty: 384 + 216 rows"),
    (600, 136, 32, "two row splits at RP = 32"),
    (776, 136, 16, "three row splits, the last of 8 rows"),
    (776, 136, 24, "three row splits at RP = 32"),
    (776, 264, 16, "three row splits over two chunks"),
    (1300, 136, 8, "four row splits launched (five asked): 3 x 384 + 148"),
    (1600, 136, 16, "five row splits launched (six asked): 4 x 384 + 64"),
    (2080, 136, 8, "six row splits launched (eight asked); gy_ = 2 (gy0_ = 4): 130 row tiles"),
    (2080, 136, 18, "gy_ = 2 at RP = 32"),
    (4100, 136, 2, "gy_ = 1, gy0_ = 2: 258 row tiles; 8 splits asked, 7 of 640 rows launched, the last of 260"),
    (4100, 136, 32, "gy_ = 1, gy0_ = 2 at RP = 32"),
    (4500, 136, 12, "8 splits launched, the last of 20 rows"),
    (64, 128, 16, "a shape the Gram chain takes under chain 0: C-space only when forced; one 128-column chunk"),
    (100, 512, 8, "forced; two whole chunks"),
    (100, 512, 32, "forced; under chain 1 a rank-32 call falls here too"),
    (576, 640, 12, "forced; two row splits of 384 + 192"),
]
# Gram six-launch chain: cfx_set_lr_chain(ctx, 1), r <= 16
GRAM = [
    (32, 128, 2, "NP = 64 from one 32-row tile: half the only tile pair is padding; KS = 2, kslab 64"),
    (32, 512, 16, "KS = 8, kslab 64"),
    (33, 256, 8, "one row past 32; KS = 4"),
    (33, 640, 12, "KS = 2, kslab 320; r != RP"),
    (64, 128, 8, "N == NP: no padding"),
    (64, 384, 16, "KS = 2, kslab 192"),
    (65, 256, 12, "one row past a 64-row tile: three tile pairs; the n0 + 64 < N step of k_lrg_v"),
    (65, 512, 2, "KS = 8 with three tile pairs"),
    (100, 128, 16, "NP = 128; r == RP = 16"),
    (100, 384, 8, "NP = 128, KS = 2"),
    (100, 640, 2, "kslab 320 at r = 2"),
    (129, 128, 8, "one row past two tiles: six tile pairs"),
    (129, 256, 16, "KS = 4, six tile pairs"),
    (129, 512, 12, "KS = 8, six tile pairs"),
    (576, 128, 8, "the tallest the chain takes: 45 tile pairs"),
    (576, 256, 2, "KS = 4 at 576 rows"),
    (576, 384, 12, "KS = 2, kslab 192 at 576 rows"),
    (576, 512, 16, "KS = 8 at 576 rows"),
    (576, 640, 8, "kslab 320 at 576 rows"),
]
GRAM_BATCHES = (1, 2, 3, 8)                           # xcd_group 8, 4, 0, 1; item 1 of a batch has no base
GRAM_BATCH_SHAPES = [(65, 256, 12), (129, 512, 16), (33, 640, 8), (100, 128, 2)]
CSPACE_BATCH_SHAPES = [(33, 136, 8), (100, 264, 18), (600, 136, 8), (31, 24, 8)]
# slab-resident chain: chain 0 on the default stream
SLAB = [
    (32, 512, 8, "one 32-row tile"),
    (32, 640, 24, "RP = 32, r != RP"),
    (33, 640, 2, "(N r) & 3 != 0: V's rows are stored two halves at a time"),
    (33, 512, 16, "one row past a tile"),
    (100, 512, 12, "r != RP = 16"),
    (100, 512, 24, "RP = 32, the blocked factorisation"),
    (100, 640, 32, "r == RP = 32"),
    (100, 640, 16, "20 slabs"),
    (576, 512, 32, "the tallest, the widest rank"),
    (576, 640, 16, "576 rows at RP = 16"),
    (576, 512, 2, "576 rows at r = 2"),
    (576, 640, 8, "576 rows at RP = 8"),
]
SLAB_BATCHES = (1, 3)
SLAB_BATCH_SHAPES = [(33, 640, 2), (100, 512, 24)]
# (form, N, C, rank, chains it runs on)
DEFICIENT = [
    ("rank3", 100, 136, 8, (2,)),
    ("rank3", 100, 512, 8, (0, 1, 2)),
    ("short", 5, 8, 8, (2,)),
    ("short", 20, 520, 32, (2,)),
    ("zero", 100, 136, 8, (2,)),
    ("zero", 100, 512, 8, (0, 1, 2)),
    ("zero", 100, 512, 32, (0, 2)),
]
# LOW_RANK_Q (even N, r % 8 == 0): (N, C, rank, lr_chain) - every chain at every RP it is built for
QUANT = [
    (100, 136, 8, 2), (600, 136, 16, 2), (100, 264, 24, 2), (776, 136, 32, 2), (100, 1032, 16, 2),
    (64, 384, 8, 1), (100, 128, 16, 1), (576, 640, 8, 1),
    (32, 512, 8, 0), (100, 640, 16, 0), (100, 512, 24, 0), (576, 512, 32, 0),
]
# the decaying spectrum keeps its 3e-3: (N, C, rank, lr_chain), the ill-conditioned case on every chain
GRADED = [(100, 512, 16, 0), (100, 512, 32, 0), (100, 512, 16, 1), (100, 512, 8, 2), (776, 264, 16, 2), (600, 136, 32, 2)]


# the draw of flat() a (N, C, rank) uses where draw 0 does not let every planted fault move the projection by 4 x its bound
# (tests/test_lr_sender_f64_host.py holds every listed case to that condition, on the draw named here)
REPS = {}
# shapes that cannot meet the condition at all, with the reason (at most one listed case in ten)
DROPPED = {}


def rep_of(N, C, rank):
    return REPS.get((N, C, rank), 0)


def all_flat_cases():
    """(chain name, lr_chain, N, C, rank, branch)"""
    out = [("cspace", 2) + c for c in CSPACE] + [("gram", 1) + c for c in GRAM] + [("slab", 0) + c for c in SLAB]
    return out
