"""Float64 witness and derived error bound of the native attention forward (cfx_attn_fwd_blocks, include/cfx.h), and the planted errors
the bound must catch.  Shared by tests/test_attn_fwd_f64.py (CPU) and tests/test_gpu_attn_fwd.py (GPU).

Witness.  From the 16-bit inputs, in float64:  s_j = scale * q . k_j  over the keys j of ALL blocks in table order (scale the fp32 value the
entry point takes),  lse = log sum_j exp(s_j),  w_j = exp(s_j - lse),  out_d = sum_j w_j v_jd.

Bound, per output element, term by term (u = 2^-24, half an fp32 ulp relative; e = 2^-11 fp16 / 2^-8 bf16, half an element ulp relative;
T = n ceil(Sk / 64) key tiles; K = 64 T keys walked, tails included):
  score accumulation   the fp32 sum of D exact products, order unknown:  (D + 2) u scale sum_d |q_d k_jd|                   }
  scale product        one rounding of acc * scale:                     u |s_j|                                             }  ds_j
  through exp          a score off by ds_j is a weight off by the factor exp(+-ds_j):  expm1(ds_j)
  exp                  x = t - m is one rounding (u |x|), the fast exponential is 2^(fp32(log2 e) x) - the constant and the product one
                       rounding each (u |x| each) - then v_exp_f32 (2 u): (3 X_j + 2) u with X_j = max_s - s_j >= |x| at any tile; the
                       rescale factors exp(m_old - m_new) of the later tiles likewise, their exponents summing to at most X_j:
                       (3 X_j + 2 T) u, common to O and l
  rescales             one rounding of O (or l) * factor per tile:  T u
                       => a weight's relative error  r_j = expm1(ds_j) + (6 X_j + 3 T + 2) u,  plus 2^-120 absolute (weights below
                       2^-126 may be flushed to zero)
  P's rounding         p, relative to the running maximum of ITS tile (so p <= 1, later scaled down), to the element type: e p_j, or
                       half a subnormal step (2^-25 fp16, 2^-134 bf16) absolute:  sum_j max(e w_j, sub / L) |v_jd|, L = sum_j exp(s_j - max_s) >= 1
  P V sum              fp32 accumulation of K products into a running O, one rounding an addition:  (K + 2) u sum_j w_j |v_jd|
  l sum                per tile 32 additions of p in a lane, then l * factor + sum (2 roundings a tile), the two halves added at the end:
                       (32 + 2 T + 2) u relative
  O / l                one correctly rounded division:  u |out_d|
  final rounding       half an ulp of the element type:  e |out_d| (or half a subnormal step)
  out bound = SLACK * [ sum_j (w_j r_j + 2^-120 + max(e w_j, sub / L)) |v_jd| + (K + 2) u W_d + W_d (sum_j w_j r_j + (32 + 2 T + 2) u) + u W_d ] + e |out_d| + sub,
              W_d = sum_j w_j |v_jd| >= |out_d|
  lse = m + log l:  the weights' errors and the l sum move log l by  sum_j w_j r_j + (32 + 2 T + 2) u;  logf: 2 u |log L| + 2 u;  the sum: u |lse|
  lse bound = SLACK * [ sum_j w_j r_j + (32 + 2 T + 2) u + 2 u (|log L| + 1) + u |lse| ]
SLACK = 2: the sums above are first order - products of two terms are dropped (expm1(ds) times P's rounding reaches 1e-4 relative in the
+-1e4 score cases) - and the internal summation order and intermediate widths of the MFMA are not documented, which the worst-case
(D + 2) and (K + 2) counts cover only if every addition rounds once.  The final half ulp of the element type is exact and not slackened.
With Gaussian unit inputs the lse bound is a few 1e-5: a lost or doubled key among 1600 moves lse by 6e-4, a lost block by 6e-2.
"""
import numpy as np

import _attn_cases as C

U = 2.0 ** -24
SLACK = 2.0
EPS = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8}
SUB = {"fp16": 2.0 ** -25, "bf16": 2.0 ** -134}          # half the smallest subnormal step


def scores(q, ks, scale):
    """float64 scores (B, H, Sq, K) over all blocks in order, and sum_d |q_d k_jd| alike"""
    qd = q.astype(np.float64).transpose(0, 2, 1, 3)
    kd = np.concatenate([k.astype(np.float64) for k in ks], axis=1).transpose(0, 2, 3, 1)
    return float(np.float32(scale)) * (qd @ kd), np.abs(qd) @ np.abs(kd)


def witness(q, ks, vs, scale):
    """out (B, Sq, H, D), lse (B, Sq, H) in float64"""
    s, _ = scores(q, ks, scale)
    m = s.max(-1, keepdims=True)
    p = np.exp(s - m)
    L = p.sum(-1, keepdims=True)
    vd = np.concatenate([v.astype(np.float64) for v in vs], axis=1).transpose(0, 2, 1, 3)
    out = (p / L) @ vd
    return out.transpose(0, 2, 1, 3), (m + np.log(L))[..., 0].transpose(0, 2, 1)


def reference_and_bound(q, ks, vs, scale, dtype):
    """(out, lse, out_bound, lse_bound) in float64"""
    e, sub = EPS[dtype], SUB[dtype]
    D, Sk, n = q.shape[-1], ks[0].shape[1], len(ks)
    T = n * ((Sk + 63) // 64)
    K = 64 * T
    s, a = scores(q, ks, scale)
    sc = float(np.float32(scale))
    m = s.max(-1, keepdims=True)
    X = m - s
    p = np.exp(-X)
    L = p.sum(-1, keepdims=True)
    w = p / L
    ds = ((D + 2) * sc * a + np.abs(s)) * U
    r = np.expm1(ds) + (6.0 * X + 3.0 * T + 2.0) * U
    lsum = (32.0 + 2.0 * T + 2.0) * U
    vd = np.concatenate([v.astype(np.float64) for v in vs], axis=1).transpose(0, 2, 1, 3)
    av = np.abs(vd)
    out = w @ vd
    W = w @ av
    wr = (w * r).sum(-1, keepdims=True)                               # sum_j w_j r_j
    tiny = 2.0 ** -120
    first = (w * r + tiny + np.maximum(e * w, sub / L)) @ av + (K + 2) * U * W + W * (wr + lsum) + U * W
    ob = SLACK * first + e * np.abs(out) + sub
    lse = (m + np.log(L))[..., 0]
    lb = SLACK * (wr[..., 0] + lsum + 2.0 * U * (np.abs(np.log(L[..., 0])) + 1.0) + U * np.abs(lse))
    return out.transpose(0, 2, 1, 3), lse.transpose(0, 2, 1), ob.transpose(0, 2, 1, 3), lb.transpose(0, 2, 1)


def check(out, lse, ref, what=""):
    """out (B, Sq, H, D), lse (B, Sq, H) against reference_and_bound's tuple: asserts, returns the largest fractions of the two bounds"""
    ro, rl, ob, lb = ref
    out, lse = np.asarray(out, dtype=np.float64), np.asarray(lse, dtype=np.float64)
    assert out.shape == ro.shape and lse.shape == rl.shape, (out.shape, ro.shape, lse.shape, rl.shape)
    assert np.isfinite(out).all() and np.isfinite(lse).all(), f"{what}: non-finite result"
    fo, fl = np.abs(out - ro) / ob, np.abs(lse - rl) / lb
    i, j = np.unravel_index(np.argmax(fo), fo.shape), np.unravel_index(np.argmax(fl), fl.shape)
    assert fo[i] <= 1.0, f"{what}: out{i} = {out[i]!r}, witness {ro[i]!r}, bound {ob[i]:.3e}: {fo[i]:.2f} x the bound"
    assert fl[j] <= 1.0, f"{what}: lse{j} = {lse[j]!r}, witness {rl[j]!r}, bound {lb[j]:.3e}: {fl[j]:.2f} x the bound"
    return float(fo[i]), float(fl[j])


def excess(out, lse, ref):
    """the largest |error| / bound over out and over lse (no assertion): what a planted error reaches"""
    ro, rl, ob, lb = ref
    with np.errstate(invalid="ignore", divide="ignore"):
        fo = np.nan_to_num(np.abs(np.asarray(out, np.float64) - ro) / ob, nan=np.inf)
        fl = np.nan_to_num(np.abs(np.asarray(lse, np.float64) - rl) / lb, nan=np.inf)
    return float(fo.max()), float(fl.max())


# ---- planted errors: what a wrong kernel would return, in float64 (the rounding to the element type left out: it is inside the bound) ----
PLANTS = ("tail", "dropblock", "twice", "noscale", "lbias", "qtail")


def can_show(plant, case):
    """Whether the case's shape and values make the planted error move the result by more than rounding - decided from the case alone,
    never from a result.  peak: the designated key holds > 0.9 of every row, the rest e^-16 each - only an error that loses or doubles
    THAT key shows.  ramp: the blocks at the top of the ramp hold everything, a block 20 below the top e^-20 - and at |s| = 1e4 the score
    term of the bound, (D + 2) u |s|, is itself of the order of one key's weight among a hundred."""
    kind, Sq, Sk, n = case["kind"], case["Sq"], case["Sk"], case["n"]
    flat = kind in ("zeroq", "equal")                  # every key weighs the same whatever the scores' scale: only v and the key COUNT matter
    pblk, pkey = C.peak_position(case) if kind == "peak" else (None, None)
    top_last = kind != "ramp" or C.RAMP[n - 1] == max(C.RAMP[:n])          # ramp: the last block is (one of) the heaviest
    if plant == "tail":                                # a last, partial key tile per block exists beside a full one
        return Sk > 64 and Sk % 64 != 0 and kind != "ramp" and (kind != "peak" or pkey >= 64 * (Sk // 64))
    if plant == "dropblock":                           # the last block is lost
        return n >= 2 and top_last and (kind != "peak" or pblk == n - 1)
    if plant == "twice":                               # block 0 is read again in the last block's place
        return n >= 2 and top_last and (kind != "peak" or pblk in (0, n - 1))
    if plant == "noscale":
        return kind != "zeroq"                         # (equal scores: out stands, lse moves)
    if plant == "lbias":                               # log(1 + 2^-8) = 3.9e-3 on lse: ten lse bounds where sum |q_d k_d| is a unit Gaussian row's
        return kind in ("gauss", "peak", "zeroq", "equal")                 # (int: |q|, |k| up to 3 make it ten times that)
    if plant == "qtail":
        return Sq % 32 != 0 and Sq > 1 and not flat    # a partial 32-row group whose zero-query tail row differs from a real row
    raise KeyError(plant)


def planted(plant, q, ks, vs, scale):
    """(out, lse) of the witness's arithmetic with one error planted"""
    if plant == "tail":
        cut = 64 * (ks[0].shape[1] // 64)
        return witness(q, [k[:, :cut] for k in ks], [v[:, :cut] for v in vs], scale)
    if plant == "dropblock":
        return witness(q, ks[:-1], vs[:-1], scale)
    if plant == "twice":
        return witness(q, [ks[0]] + list(ks[1:-1]) + [ks[0]], [vs[0]] + list(vs[1:-1]) + [vs[0]], scale)      # block 0 read again for the last
    if plant == "noscale":
        return witness(q, ks, vs, 1.0)
    if plant == "lbias":
        out, lse = witness(q, ks, vs, scale)
        return out / (1.0 + 2.0 ** -8), lse + np.log1p(2.0 ** -8)
    if plant == "qtail":
        out, lse = witness(q, ks, vs, scale)
        zo, zl = witness(np.zeros_like(q[:, :1]), ks, vs, scale)     # what a tail row computes: zero queries
        out, lse = out.copy(), lse.copy()
        out[:, -1], lse[:, -1] = zo[:, 0], zl[:, 0]                  # ... stored over the last real row
        return out, lse
    raise KeyError(plant)
