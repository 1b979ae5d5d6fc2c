"""The ring-attention block merge (cfx_attn_merge, cfx_attn_merge_wait, cfx_attn_merge_ex) against its published formula in float64,
with an error bound DERIVED from the inputs - a helper, not a test; shared by tests/test_attn_merge_f64.py (CPU) and
tests/test_gpu_attn_merge_f64.py (GPU).

Reference, block by block on the fp32-widened inputs, in float64 (the first block initialises):
    x = lse_b - lse ;  sg = sigmoid(x) ;  out <- out - sg * (out - out_b) ;  lse <- lse + softplus(x)      (= lse - logsigmoid(lse - lse_b))

Bound (u = 2^-24, half an fp32 ulp relative; Eo, El the errors carried by out and lse so far, 0 after the first block, which is exact):
  x      one fp32 subtraction of the carried lse:                      dx  = El + u (|x| + El)
  exp    the kernel's __expf(t) is v_exp_f32(fp32(log2 e) * t) (__clang_hip_math.h): one ulp for the instruction plus the rounded
         product carried into the exponent,                            rho = 2^-23 + 1.5 |x| 2^-24  relative (the eager formula's
         exponential, 1 ulp, lies inside it)
  sg     1 / (1 + e): e is wrong by rho, x by dx, then one rounding for the add and one for the divide.  To first order that is
         sg (1 - sg) (dx + rho) + 2 u sg; it is evaluated at the ends of the interval instead (sigmoid is monotone), which needs no
         second-order allowance:
                                                                       sg_hi = 1 / (1 + exp(-(x + dx)) (1 - rho))
                                                                       sg_lo = 1 / (1 + exp(-(x - dx)) (1 + rho))
                                                                       dsg = max(sg_hi - sg, sg - sg_lo) + 2 u sg_hi
  out    with out~ = out + eps: out~ - sg~ (out~ - out_b) - (out - sg d) = eps (1 - sg~) - (sg~ - sg) d, d = out - out_b: the carried
         error passes undiminished at worst (a convex combination), the sigmoid's error is scaled by |d|; then the three roundings of
         the update - the difference (scaled by sg) and the product, 2 u p with p = sg_hi (|d| + Eo), and the final subtraction,
         which moves its result by at most u |out'| and never by more than the subtrahend itself (out~ is an fp32 number: the
         rounded difference is at least as near):
                                                                       Eo' = Eo + dsg (|d| + Eo) + 2 u p + min(u (|out'| + Eo), p)
  lse    lse~ + softplus(x~) - lse - softplus(x) = eps_l (1 - sg(xi)) + sg(xi) r with r the rounding of x: El + sg_hi u (|x| + El);
         log1p(e) with e wrong by rho moves by e / (1 + e) rho, its own evaluation by 2 ulp (4 u log1p(e)); one rounding of
         q = max(x, 0) + log1p(e) and one of the final sum, again no larger than what is added:
                                                                       El' = El + u (sg_hi (|x| + El) + q) + min(u (|lse'| + El), q + sg_hi dx)
                                                                                + e / (1 + e) rho + 4 u log1p(e)
  Both get a factor 1 + 2^-10 on the rounding terms (products of two relative errors) and 2^-120 absolute (results below fp32's normal
  range: an exponential that overflows to inf or underflows to 0 leaves sg, log1p(e) off by less than that).
The bound grows with |lse| and |lse_b| through dx (El is at least u |lse|), as the eager fp32 formula's measured error does."""
import zlib

import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -120
SLACK = 1.0 + 2.0 ** -10
F32, F64 = np.float32, np.float64


def rho_fast(ax):
    return 2.0 ** -23 + 1.5 * ax * 2.0 ** -24


def _exp(t):
    with np.errstate(over="ignore", under="ignore"):
        return np.exp(t)


def step64(o, l, ob, lb):
    """one merge step in float64: (out', lse', sg, x)"""
    x = lb - l
    sg = 1.0 / (1.0 + _exp(-x))
    return o - sg[..., None] * (o - ob), l + (np.maximum(x, 0.0) + np.log1p(_exp(-np.abs(x)))), sg, x


def reference_and_bound(blocks, rho=rho_fast):
    """blocks: [(out_b (B,S,H,D), lse_b (B,S,H))] as fp32 arrays (the widened inputs).  Returns (out, lse, Eo, El) in float64."""
    o, l = blocks[0][0].astype(F64), blocks[0][1].astype(F64)
    Eo, El = np.zeros_like(o), np.zeros_like(l)
    for ob, lb in blocks[1:]:
        ob, lb = ob.astype(F64), lb.astype(F64)
        o2, l2, sg, x = step64(o, l, ob, lb)
        ax = np.abs(x)
        dx = El + U * (ax + El)
        r = rho(ax + dx)
        sg_hi = 1.0 / (1.0 + _exp(-(x + dx)) * (1.0 - r))
        sg_lo = 1.0 / (1.0 + _exp(-(x - dx)) * (1.0 + r))
        dsg = np.maximum(sg_hi - sg, sg - sg_lo) + 2.0 * U * sg_hi
        d = np.abs(o - ob)
        p = sg_hi[..., None] * (d + Eo)
        Eo = Eo + dsg[..., None] * (d + Eo) + SLACK * (2.0 * U * p + np.minimum(U * (np.abs(o2) + Eo), p)) + TINY
        e = _exp(-(ax - dx))
        q = l2 - l
        El = (El + SLACK * (U * (sg_hi * (ax + El) + q) + np.minimum(U * (np.abs(l2) + El), q + sg_hi * dx)) + e / (1.0 + e) * r
              + 4.0 * U * np.log1p(e) + TINY)
        o, l = o2, l2
    return o, l, Eo, El


def check(out32, lse32, blocks, what="merge", rho=rho_fast):
    """AssertionError unless out32 / lse32 (fp32, (B,S,H,D) / (B,S,H)) lie within the bound of the float64 reference.  Returns the worst
    error as a fraction of the bound: (out, lse)."""
    o, l, Eo, El = reference_and_bound(blocks, rho)
    out32, lse32 = np.asarray(out32), np.asarray(lse32)
    assert out32.dtype == F32 and lse32.dtype == F32 and out32.shape == o.shape and lse32.shape == l.shape, (out32.dtype, out32.shape, o.shape)
    assert np.isfinite(out32).all() and np.isfinite(lse32).all(), f"{what}: non-finite result"
    if len(blocks) == 1:
        assert np.array_equal(out32.astype(F64), o) and np.array_equal(lse32.astype(F64), l), f"{what}: a single block is copied exactly"
        return 0.0, 0.0
    fo = np.abs(out32.astype(F64) - o) / Eo
    fl = np.abs(lse32.astype(F64) - l) / El
    bad = fo > 1.0
    assert not bad.any(), (f"{what}: out: {int(bad.sum())}/{bad.size} beyond the bound (worst {fo.max():.3g} x the bound at "
                           f"{tuple(int(i) for i in np.unravel_index(np.argmax(fo), fo.shape))})")
    bad = fl > 1.0
    assert not bad.any(), (f"{what}: lse: {int(bad.sum())}/{bad.size} beyond the bound (worst {fl.max():.3g} x the bound at "
                           f"{tuple(int(i) for i in np.unravel_index(np.argmax(fl), fl.shape))})")
    return float(fo.max()), float(fl.max())


# ---- the two fp32 forms a CPU can run -------------------------------------------------------------------------------------------------
def eager_fp32(blocks):
    """the published formula in eager fp32 torch, as tests/test_gpu_api.py writes it"""
    import torch.nn.functional as Fn
    o = l = None
    for ob, lb in blocks:
        ob, lb = torch.from_numpy(ob), torch.from_numpy(lb).unsqueeze(-1)
        if o is None:
            o, l = ob, lb
        else:
            o, l = o - torch.sigmoid(lb - l) * (o - ob), l - Fn.logsigmoid(l - lb)
    return o.numpy(), l.squeeze(-1).numpy()


def kernel_fp32(blocks, exp_err=0.0, merge=None):
    """attn_merge_body transcribed to numpy fp32, operation for operation; its two exponentials are the exact ones moved by exp_err x rho
    relative (+1 / -1: the stated error of __expf in either direction).  merge(o, l, ob, lb, k) -> (o', l') replaces a step (planted
    errors)."""
    def fexp(t):
        e = _exp(t.astype(F64))
        with np.errstate(over="ignore"):
            return (e * (1.0 + exp_err * rho_fast(np.abs(t.astype(F64))))).astype(F32)

    def body(o, l, ob, lb):
        x = lb - l
        sg = F32(1.0) / (F32(1.0) + fexp(-x))
        o2 = o - sg[..., None] * (o - ob)
        l2 = l + (np.maximum(x, F32(0.0)) + np.log1p(fexp(-np.abs(x)).astype(F64)).astype(F32))
        return o2, l2
    o, l = blocks[0][0].copy(), blocks[0][1].copy()
    for k, (ob, lb) in enumerate(blocks[1:], 1):
        with np.errstate(over="ignore", under="ignore"):
            o, l = body(o, l, ob, lb) if merge is None else merge(body, o, l, ob, lb, k)
        assert o.dtype == F32 and l.dtype == F32
    return o, l


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
HEAD_DIMS = (8, 16, 24, 40, 72, 128, 136, 264, 512)      # 1 .. 64 lanes a row; 3, 5, 9, 17, 33 lanes leave idle lanes in the group
GAPS = {"zero": (0.0, 2.0 ** -20, -2.0 ** -20), "unit": (1.0, -1.0), "mid": (20.0, -20.0), "far": (90.0, -90.0), "huge": (1e4, -1e4)}
FLUX = (1, 4608, 24, 128)


def _cases():
    out = []
    i = 0
    classes = list(GAPS)
    for D in HEAD_DIMS:
        # rows = B S H: 42 rows x 2^lg lanes is no multiple of 256 for any lg <= 6; 256 rows is one for every lg
        for shape in ((2, 7, 3), (2, 16, 8)):
            out.append(dict(dtype=("fp16", "bf16")[i % 2], shape=shape + (D,), n=(2, 4, 15)[i % 3], gap=classes[i % 5],
                            offset=(0.0, 300.0, -300.0)[(i // 2) % 3], mag="unit"))
            i += 1
    for D in (24, 136):
        for shape, why in (((3, 1, 5), "S = 1"), ((2, 9, 1), "H = 1"), ((1, 5, 3), "B = 1")):
            for dtype in ("fp16", "bf16"):
                out.append(dict(dtype=dtype, shape=shape + (D,), n=4, gap=classes[i % 5], offset=(300.0, -300.0, 0.0)[i % 3], mag="unit"))
                i += 1
    for dtype in ("fp16", "bf16"):
        for gap in classes:              # every gap class with both element types, values at the top of the type's range
            out.append(dict(dtype=dtype, shape=(1, 6, 3, 72), n=4, gap=gap, offset=0.0, mag="max"))
            out.append(dict(dtype=dtype, shape=(2, 5, 2, 40), n=2, gap=gap, offset=(300.0 if gap in ("zero", "mid") else -300.0), mag="unit"))
    out.append(dict(dtype="bf16", shape=FLUX, n=2, gap="unit", offset=0.0, mag="unit"))
    for k, c in enumerate(out):
        B, S, H, D = c["shape"]
        c["id"] = f"{c['dtype']}-{B}x{S}x{H}x{D}-n{c['n']}-{c['gap']}-off{int(c['offset'])}-{c['mag']}"
    return out


CASES = _cases()


def build(case):
    """[(out_b fp32 (B,S,H,D) holding values of the case's element type, lse_b fp32 (B,S,H))]: block k's lse is the running lse plus the
    class's gap, as far as fp32 can say it.  The gap's sign alternates across rows and, except in every third row, along the chain.  In
    chains of 4 and more blocks of the classes `far` and `huge` block 1 comes at a unit gap: at those gaps the sigmoid is exactly 0 or 1,
    the merge copies, and only a state that already carries fp32 roundings shows whether a later step keeps them."""
    B, S, H, D = case["shape"]
    rng = np.random.default_rng(zlib.crc32(case["id"].encode()))
    tdt = torch.float16 if case["dtype"] == "fp16" else torch.bfloat16
    top = 65504.0 if case["dtype"] == "fp16" else 2.0 ** 100
    gaps = GAPS[case["gap"]]
    blocks = []
    l = None
    for k in range(case["n"]):
        v = rng.standard_normal((B, S, H, D)).astype(F32)
        if case["mag"] == "max":
            v = (rng.uniform(-1.0, 1.0, (B, S, H, D)) * top).astype(F32)
            v.reshape(-1)[::7] = top
            v.reshape(-1)[3::11] = -top
        ob = torch.from_numpy(v).to(tdt).to(torch.float32).numpy()
        if l is None:
            lb = (case["offset"] + rng.standard_normal((B, S, H))).astype(F32)
            l = lb.astype(F64)
        else:
            row = np.arange(B * S * H).reshape(B, S, H)
            g = GAPS["unit"] if k == 1 and case["n"] >= 4 and case["gap"] in ("far", "huge") else gaps
            lb = (l + np.asarray(g)[(row + k * (row % 3 != 0)) % len(g)]).astype(F32)
            l = step64(np.zeros((B, S, H, 1)), l, np.zeros((B, S, H, 1)), lb.astype(F64))[1]
        blocks.append((ob, lb))
    return blocks
