"""The one-launch merge of all of a layer's attention blocks (cfx_attn_merge_many, compact/attention.py merge_blocks) against the direct
softmax-weighted formula in float64, with an error bound DERIVED from the inputs and n - a helper, not a test; shared by
tests/test_attn_merge_many_f64.py (CPU) and tests/test_gpu_attn_merge_many.py (GPU).  Inputs come from tests/_merge_f64.py (build, CASES).

Witness, on the fp32-widened inputs, in float64 - the direct formula, independent of _merge_f64's chain:
    m = max_i l_i ;  e_i = exp(l_i - m) ;  Z = sum_i e_i ;  out_d = (sum_i e_i o_id) / Z ;  lse = m + log Z

What the launch computes (include/cfx.h), each operation rounded once in fp32:
    x_i = l_i - m ;  e_i = __expf(x_i) ;  Z = ((e_0 + e_1) + ...) ;  a_d = ((e_0 o_0d + e_1 o_1d) + ...) ;  out_d = a_d / Z ;  lse = m + logf(Z)

Bound (u = 2^-24, half an fp32 ulp relative; the maximum m is one of the inputs: exact):
  x_i    one fp32 subtraction: off by at most u |x_i|, which the exponential carries as the factor exp(+-u |x_i|).
  e_i    __expf is v_exp_f32(fp32(log2 e) * t): rho_fast(|t|) relative (tests/_merge_f64.py), at the rounded argument |x_i| (1 + u).  Together
                                                                       eta_i = exp(u |x_i|) (1 + rho_fast(|x_i| (1 + u))) - 1   relative,
         and tau = 2^-126 absolute for an exponential that underflows or is flushed to 0:
                                                                       dE_i = eta_i e_i + tau
         For x_i = 0 - the maximum, and every tie with it - the subtraction gives 0 and the exponential exactly 1: dE_i = 0.
  Z      n - 1 additions in index order: term i passes at most n - 1 of them, g1 = (1 + u)^(n-1) - 1 relative:
                                                                       EZ = (1 + g1) sum_i dE_i + g1 Z
  a_d    one rounding per product and the same n - 1 additions, g = (1 + u)^n - 1 relative on each term; a product or partial sum below
         fp32's normal range may be flushed, 2^-126 each (2 n of them):
                                                                       EA_d = sum_i |o_id| (dE_i (1 + g) + e_i g) + 2 n 2^-126
         (tau inside dE_i, times |o_id|, is the absolute term 2^-126 sum_i |o_id| of the underflowing exponentials)
  out_d  a quotient of two inexact numbers, then ONE rounding (a correctly rounded division, no reciprocal); Z >= 1 > EZ:
                                                                       q_d  = (EA_d + |out_d| EZ) / (Z - EZ)
                                                                       Eo_d = q_d + u (|out_d| + q_d)
  lse    log is 1 / Z-Lipschitz at Z >= 1: the error of Z moves it by at most EZ / (Z - EZ); logf is granted 2 ulp of its result
         (4 u relative, as _merge_f64 grants log1p); then the final addition rounds once:
                                                                       EL = EZ / (Z - EZ) + 4 u (log Z + EZ / (Z - EZ))
                                                                       El = EL + u (|lse| + EL)
  The rounding terms (g1, g, u, 4 u) are taken times 1 + 2^-10, as in _merge_f64: rho_fast is a first-order figure, and the bound itself is
  evaluated in float64.  TINY = 2^-120 absolute is added to both (results below fp32's normal range).
The bound is a function of the inputs and n only.  n = 1 is held to EXACT equality, not to the bound."""
import numpy as np

from _merge_f64 import F32, F64, SLACK, TINY, U, _exp, rho_fast

TAU = 2.0 ** -126


def witness(blocks):
    """blocks: [(out_b (B,S,H,D), lse_b (B,S,H))] fp32 arrays (the widened inputs) -> (out, lse, e (n,B,S,H), Z, m) in float64"""
    o = np.stack([b[0].astype(F64) for b in blocks])
    l = np.stack([b[1].astype(F64) for b in blocks])
    m = l.max(axis=0)
    e = _exp(l - m)
    Z = e.sum(axis=0)
    out = (e[..., None] * o).sum(axis=0) / Z[..., None]
    return out, m + np.log(Z), e, Z, m


def witness_and_bound(blocks, rho=rho_fast):
    """(out, lse, Eo, El) in float64"""
    n = len(blocks)
    out, lse, e, Z, m = witness(blocks)
    ao = np.stack([np.abs(b[0].astype(F64)) for b in blocks])
    ax = np.abs(np.stack([b[1].astype(F64) for b in blocks]) - m)
    eta = _exp(U * ax) * (1.0 + rho(ax * (1.0 + U))) - 1.0
    dE = np.where(ax == 0.0, 0.0, eta * e + TAU)
    g1 = SLACK * ((1.0 + U) ** (n - 1) - 1.0)
    g = SLACK * ((1.0 + U) ** n - 1.0)
    EZ = (1.0 + g1) * dE.sum(axis=0) + g1 * Z
    EA = (ao * (dE * (1.0 + g) + e * g)[..., None]).sum(axis=0) + 2.0 * n * TAU
    q = (EA + np.abs(out) * EZ[..., None]) / (Z - EZ)[..., None]
    Eo = q + SLACK * U * (np.abs(out) + q) + TINY
    dl = EZ / (Z - EZ)
    EL = dl + SLACK * 4.0 * U * (np.log(Z) + dl)
    El = EL + SLACK * U * (np.abs(lse) + EL) + TINY
    return out, lse, Eo, El


def check(out32, lse32, blocks, what="merge_many", rho=rho_fast):
    """AssertionError unless out32 / lse32 (fp32, (B,S,H,D) / (B,S,H)) lie within the bound of the float64 witness; a single block must
    come back exactly.  Returns the worst error as a fraction of the bound: (out, lse)."""
    o, l, Eo, El = witness_and_bound(blocks, rho)
    out32, lse32 = np.asarray(out32), np.asarray(lse32)
    assert out32.dtype == F32 and lse32.dtype == F32 and out32.shape == o.shape and lse32.shape == l.shape, (out32.dtype, out32.shape, o.shape)
    assert np.isfinite(out32).all() and np.isfinite(lse32).all(), f"{what}: non-finite result"
    if len(blocks) == 1:
        assert np.array_equal(out32, blocks[0][0]) and np.array_equal(lse32, blocks[0][1]), f"{what}: a single block is returned exactly"
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


PLANTS = ("drop", "swap", "zmiss", "nomax", "fp16sum")


def kernel_fp32(blocks, exp_err=0.0, plant=None):
    """k_attn_merge_many transcribed to numpy fp32, operation for operation; its exponentials are the exact ones moved by exp_err x rho
    relative (+1 / -1: the stated error of __expf in either direction; exactly 1 at 0, as the instruction gives).  plant: one of PLANTS -
    a dropped block (block 1), the lse of blocks 0 and 1 swapped, Z without its last term, the maximum not subtracted, the sum kept in
    fp16."""
    def fexp(t):
        t64 = t.astype(F64)
        with np.errstate(over="ignore"):
            return np.where(t64 == 0.0, 1.0, _exp(t64) * (1.0 + exp_err * rho_fast(np.abs(t64)))).astype(F32)

    os_ = [b[0] for b in blocks]
    ls = [b[1] for b in blocks]
    if plant == "drop" and len(blocks) > 1:
        os_, ls = os_[:1] + os_[2:], ls[:1] + ls[2:]
    if plant == "swap" and len(blocks) > 1:
        ls = [ls[1], ls[0]] + ls[2:]
    m = ls[0]
    for l in ls[1:]:
        m = np.maximum(m, l)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        es = [fexp(l if plant == "nomax" else l - m) for l in ls]
        Z = es[0]
        for e in (es[1:-1] if plant == "zmiss" and len(es) > 1 else es[1:]):
            Z = Z + e
        acc_t = np.float16 if plant == "fp16sum" else F32
        a = (es[0][..., None] * os_[0]).astype(acc_t)
        for e, o in zip(es[1:], os_[1:]):
            a = (a + (e[..., None] * o).astype(acc_t)).astype(acc_t)
        out = a.astype(F32) / Z[..., None]
        lse = ((F32(0.0) if plant == "nomax" else m) + np.log(Z.astype(F64)).astype(F32)).astype(F32)
    assert out.dtype == F32 and lse.dtype == F32
    return out, lse
