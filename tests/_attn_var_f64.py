"""Float64 witness and derived error bound of the native attention forward over K,V blocks of UNEQUAL length (cfx_attn_fwd_blocks_var,
include/cfx.h), and the planted errors the bound must catch.  Shared by tests/test_attn_var_f64.py (CPU) and tests/test_gpu_attn_var.py (GPU).

The witness, the check and the excess are those of tests/_attn_f64.py (`scores`, `witness`, `check`, `excess`: they concatenate blocks of
any length).  The bound is `_attn_f64.reference_and_bound`'s, term by term, with the ONE thing that changes: the launch walks
    T = sum_i ceil(Sk_i / 64)   key tiles,   K = 64 T   keys, tails included
(a tile never straddles a block), where the equal-length launch walks n ceil(Sk / 64).  No new constant: U, EPS, SUB and SLACK = 2 are
_attn_f64's, for the reasons stated there.  On equal lengths the two bounds are the same numbers.
"""
import numpy as np

import _attn_cases as C
import _attn_f64 as W
import _attn_var_cases as V
from _attn_f64 import check, excess, scores, witness  # noqa: F401  (re-exported: one witness, one check)

U, SLACK, EPS, SUB = W.U, W.SLACK, W.EPS, W.SUB


def tiles(sks):
    return sum((int(n) + 63) // 64 for n in sks)


def reference_and_bound(q, ks, vs, scale, dtype):
    """(out, lse, out_bound, lse_bound) in float64: _attn_f64.reference_and_bound with T = sum_i ceil(Sk_i / 64)"""
    e, sub = EPS[dtype], SUB[dtype]
    D = q.shape[-1]
    T = tiles(k.shape[1] for k in ks)
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
    Wd = w @ av
    wr = (w * r).sum(-1, keepdims=True)
    tiny = 2.0 ** -120
    first = (w * r + tiny + np.maximum(e * w, sub / L)) @ av + (K + 2) * U * Wd + Wd * (wr + lsum) + U * Wd
    ob = SLACK * first + e * np.abs(out) + sub
    lse = (m + np.log(L))[..., 0]
    lb = SLACK * (wr[..., 0] + lsum + 2.0 * U * (np.abs(np.log(L[..., 0])) + 1.0) + U * np.abs(lse))
    return out.transpose(0, 2, 1, 3), lse.transpose(0, 2, 1), ob.transpose(0, 2, 1, 3), lb.transpose(0, 2, 1)


# ---- planted errors: what a kernel (or a caller) with ONE index wrong would return, in float64 -------------------------------------------
# A table slot i READS `length` keys of the data of block `d`, batch b starting `stride` keys * b into d's buffer; what lies past the
# buffer's end is modelled as zeros (zero K: score 0, zero V) - the LEAST visible thing a wild read can return.
PLANTS = ("mask_next", "mask_prev", "stride0", "droplast", "jointend")


def _read(x, length, stride):
    B, n, H, D = x.shape
    rows = np.concatenate([x.reshape(B * n, H, D), np.zeros((max(0, (B - 1) * stride + length - B * n), H, D), x.dtype)], axis=0)
    return np.stack([rows[b * stride:b * stride + length] for b in range(B)])


def _masked(k, v, own, eff):
    """block of `own` keys whose scores are masked with length `eff`: eff < own loses the keys from eff on; eff > own scores the zero
    rows the staging wrote, up to the end of the block's last tile, as real keys (score 0, V = 0)"""
    if eff <= own:
        return k[:, :eff], v[:, :eff]
    extra = min(eff, 64 * ((own + 63) // 64)) - own
    z = np.zeros((k.shape[0], extra) + k.shape[2:], k.dtype)
    return np.concatenate([k, z], axis=1), np.concatenate([v, z], axis=1)


def _changed_keys(sks, eff):
    """keys lost or wrongly gained by masking block i with eff[i]"""
    return sum(n - e if e <= n else min(e, 64 * ((n + 63) // 64)) - n for n, e in zip(sks, eff))


def _neighbour(sks, plant):
    return [sks[min(i + 1, len(sks) - 1)] for i in range(len(sks))] if plant == "mask_next" else [sks[max(i - 1, 0)] for i in range(len(sks))]


def _peak_seen(B, n_data, pkey, length, stride):
    """how often batch b's window of `length` keys, `stride` * b keys into the data block of n_data keys a batch, holds a designated key
    (one per batch, at pkey): a list over b.  Anything but exactly once moves the row by the order of its values (lost) or lse by log 2"""
    peaks = [bb * n_data + pkey for bb in range(B)]
    return [sum(b * stride <= p < b * stride + length for p in peaks) for b in range(B)]


def can_show(plant, case):
    """Whether the case's lengths and values make the planted error move the result by more than rounding - decided from the case alone,
    never from a result.  gauss: every key weighs about 1 / K of a row (K <= 384 here), a lost, gained or exchanged key moves lse by about
    that: three orders above the bound of a few 1e-5.  peak: the designated key holds > 0.9 of every row, the rest e^-16 each - only an
    error that loses, doubles or misplaces THAT key shows.  ramp: the blocks at the top of the ramp hold everything - only the loss of a
    heaviest block shows (as _attn_f64.can_show has it)."""
    kind, B, sks = case["kind"], case["B"], case["sks"]
    n = len(sks)
    pblk, pkey = V.peak_position(case) if kind == "peak" else (None, None)
    if plant in ("mask_next", "mask_prev"):             # every block's scores masked with its neighbour's length
        eff = _neighbour(sks, plant)
        if kind == "ramp":
            return False
        if kind == "peak":
            return pkey >= eff[pblk]                    # the designated key itself is masked away
        return _changed_keys(sks, eff) >= 1
    if plant == "stride0":                              # block 0's batch stride for every block: batch 1 reads elsewhere
        if B < 2 or kind == "ramp":
            return False
        if kind == "peak":
            return _peak_seen(B, sks[pblk], pkey, sks[pblk], sks[0]) != [1] * B
        return any(s != sks[0] for s in sks)
    if plant == "droplast":
        if kind == "ramp":
            return n >= 2 and C.RAMP[n - 1] == max(C.RAMP[:n])           # the last block is (one of) the heaviest
        return n >= 2 and (kind != "peak" or pblk == n - 1)
    if plant == "jointend":                             # the pointers of [joint, rest...] as [rest..., joint], the lengths left where they were
        if kind == "ramp" or sks[1:] + sks[:1] == sks:
            return False
        if kind == "peak":                              # slot i reads the data of block (i + 1) % n with its own length and stride
            i = (pblk - 1) % n
            return _peak_seen(B, sks[pblk], pkey, sks[i], sks[i]) != [1] * B
        return True
    raise KeyError(plant)


def planted(plant, q, ks, vs, scale):
    """(out, lse) of the witness's arithmetic with one error planted"""
    sks = [k.shape[1] for k in ks]
    n = len(ks)
    if plant in ("mask_next", "mask_prev"):
        kv = [_masked(k, v, own, eff) for k, v, own, eff in zip(ks, vs, sks, _neighbour(sks, plant))]
        return witness(q, [a for a, _ in kv], [b for _, b in kv], scale)
    if plant == "stride0":
        return witness(q, [_read(k, s, sks[0]) for k, s in zip(ks, sks)], [_read(v, s, sks[0]) for v, s in zip(vs, sks)], scale)
    if plant == "droplast":
        return witness(q, ks[:-1], vs[:-1], scale)
    if plant == "jointend":
        return witness(q, [_read(ks[(i + 1) % n], sks[i], sks[i]) for i in range(n)], [_read(vs[(i + 1) % n], sks[i], sks[i]) for i in range(n)], scale)
    raise KeyError(plant)
