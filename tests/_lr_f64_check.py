"""The float64 witness of the low-rank RECEIVER: out = base + fp16(U V) (csrc/cfx_lowrank.hip k_lr_decode, k_lr_decode_mfma, the slab
chain's fused update) and the int4 factor dequantiser in front of it (k_lr_dq4) - element by element.  A plain module: numpy only, no
code shared with tests/_oracle_backend.py, nothing of the library is called.

    bounds(U, V, base)               -> (lo, hi) fp16 arrays (N, C)
    check(U, V, base, out, what)     -> pinned share; asserts lo <= out <= hi element by element
    split_q(packet, N, C, r)         -> (Uq (N, r), Vq (r, C)) fp16: the LOW_RANK_Q packet dequantised by the definition
    check_q(packet, N, C, r, base, out, what) -> pinned share

U (N, r), V (r, C), base (N, C) or None, out (N, C): fp16 arrays or their uint16 bits.

The bound.  p = U V and S = |U| |V| in float64 (exact to 2^-53: nothing beside what follows), e = (r + 1) 2^-23 S.  The products of two fp16
numbers are exact in fp32; a kernel then makes at most r additions in fp32, in whatever order; an addition, rounded to nearest or
truncated, loses at most 2^-23 of its result, and no partial sum exceeds S: the fp32 sum a kernel rounds to fp16 lies within e of p.  This
covers the v_dot2 chain, the MFMA order and the slab chain's fused form without saying how each of them sums.  Where no addition can
round at all - every product of the element is a multiple of one power of two q (from the trailing zero bits of the row of U and the
column of V) and S <= 2^24 q, so that every partial sum in any order is a multiple of q within fp32's 24 bits - e is 0: that is what
makes the `integers` case bit for bit although its sums cancel.  Rounding is monotone, so

    lo = fp16(base + fp16(p - e))  <=  out  <=  hi = fp16(base + fp16(p + e))          (no base: fp16(p -+ e))

with every conversion the correctly rounded one - the kernels claim one rounding to fp16 and one fp16 add.  Zeros are equal whatever
their sign, and nothing in the domain is non-finite: lo, hi and out must be finite.  Where lo == hi the element is PINNED: the kernel
has to produce exactly that value.  An interval test that pins little proves little, so callers hold the pinned share
(tests/test_lr_f64_host.py: >= 80 % on every random draw the GPU tests use, 100 % on the exact cases).

Subnormal factor entries: v_dot2 and the MFMA units may flush an fp16 subnormal operand to zero, and the library does not say which
they do; the bound of an element is widened by the |u_k v_k| of every term with a subnormal factor in it.

LOW_RANK_Q (include/cfx.h): [int4(U) (N/2, r) | scale r | min r | int4(V^T) (C/2, r) | scale r | min r], low nibble = even row;
a factor entry is fp16(fp16(q * scale) + min) - two roundings."""
import numpy as np

F16, F64 = np.float16, np.float64
EPS32 = 2.0 ** -23


def f16(a):
    a = np.asarray(a)
    return a.view(F16) if a.dtype == np.uint16 else a.astype(F16, copy=False)


def _subnormal(a16):
    u = a16.view(np.uint16) & 0x7FFF
    return (u > 0) & (u < 0x0400)


def _quantum(a16):
    """the power of two an fp16 value is an odd multiple of (zero: infinity)"""
    b = a16.view(np.uint16).astype(np.int64)
    ex, mant = (b >> 10) & 0x1F, b & 0x3FF
    m = np.where(ex == 0, mant, mant | 0x400)
    e2 = np.where(ex == 0, -24, ex - 25)
    low = (m & -m).astype(F64)
    with np.errstate(divide="ignore"):
        return np.where(m == 0, np.inf, low * np.exp2(e2.astype(F64)))


def bounds(U, V, base=None):
    U, V = f16(U), f16(V)
    N, r = U.shape
    assert V.shape[0] == r, (U.shape, V.shape)
    u, v = U.astype(F64), V.astype(F64)
    assert np.isfinite(u).all() and np.isfinite(v).all(), "non-finite factor entries are outside the domain"
    p = u @ v
    au, av = np.abs(u), np.abs(v)
    S = au @ av
    # no addition rounds where every product of the element is a multiple of one power of two q and S <= 2^24 q: every partial sum, in
    # any order, is then a multiple of q that the 24 bits of fp32 hold
    q = _quantum(U).min(axis=1)[:, None] * _quantum(V).min(axis=0)[None, :]
    with np.errstate(invalid="ignore"):
        e = np.where(S <= 2.0 ** 24 * q, 0.0, (r + 1) * EPS32 * S)
    su, sv = _subnormal(U), _subnormal(V)
    if su.any() or sv.any():
        e = e + (au * su) @ av + (au * ~su) @ (av * sv)
    with np.errstate(over="ignore"):
        lo, hi = (p - e).astype(F16), (p + e).astype(F16)
        if base is not None:
            b = f16(base).astype(F64).reshape(N, -1)
            lo, hi = (b + lo.astype(F64)).astype(F16), (b + hi.astype(F64)).astype(F16)
    return lo, hi


def check(U, V, base, out, what=""):
    lo, hi = bounds(U, V, base)
    o = f16(out).reshape(lo.shape)
    assert np.isfinite(lo).all() and np.isfinite(hi).all(), f"{what}: the case leaves the finite domain"
    fin = np.isfinite(o)
    assert fin.all(), f"{what}: {int((~fin).sum())} non-finite elements (first at {tuple(np.argwhere(~fin)[0])})"
    o64, lo64, hi64 = o.astype(F64), lo.astype(F64), hi.astype(F64)
    bad = (o64 < lo64) | (o64 > hi64)
    if bad.any():
        n, c = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.size} elements outside [lo, hi]; first at ({n}, {c}): got {o64[n, c]!r} "
                             f"({int(o.view(np.uint16)[n, c]):#06x}), lo {lo64[n, c]!r}, hi {hi64[n, c]!r}; rows {np.unique(np.argwhere(bad)[:, 0])[:8].tolist()}")
    return float((lo64 == hi64).mean())


def pinned_share(U, V, base=None):
    lo, hi = bounds(U, V, base)
    return float((lo.astype(F64) == hi.astype(F64)).mean())


def _dq_section(sec, rows, r):
    """[codes (rows/2, r) u8 | scale r | min r] -> (rows, r) fp16 by the definition, in float64 with two fp16 roundings"""
    sec = np.ascontiguousarray(sec).view(np.uint8)
    assert sec.size == rows * r // 2 + 4 * r, (sec.size, rows, r)
    codes = sec[:rows * r // 2].reshape(rows // 2, r)
    sm = sec[rows * r // 2:].copy().view(F16).astype(F64)
    scale, mn = sm[:r], sm[r:]
    q = np.empty((rows, r), F64)
    q[0::2] = codes & 0x0F
    q[1::2] = codes >> 4
    with np.errstate(over="ignore", invalid="ignore"):
        return ((q * scale[None, :]).astype(F16).astype(F64) + mn[None, :]).astype(F16)


def split_q(packet, N, C, r):
    b = np.ascontiguousarray(packet).reshape(-1).view(np.uint8)
    nu, nv = N * r // 2 + 4 * r, C * r // 2 + 4 * r
    assert b.size == nu + nv, (b.size, nu + nv)
    return _dq_section(b[:nu], N, r), np.ascontiguousarray(_dq_section(b[nu:], C, r).T)


def check_q(packet, N, C, r, base, out, what=""):
    Uq, Vq = split_q(packet, N, C, r)
    return check(Uq, Vq, base, out, what)
