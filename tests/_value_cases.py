"""The VALUE domain of the int8, int4 and top-k codecs as deterministic cases - a plain module in the manner of tests/_bf16_cases.py, shared
by tests/test_value_domain_f64.py (CPU: the oracles against the definition, and the proof that every case holds what its `why` says) and
tests/test_gpu_value_domain.py (GPU: every launch form against the oracle and the definition).  Every case stays inside the documented
domain: finite values, |x - base| < 65504 (`range-overflow` is finite too: only fp16(max - min) is not).

    CASES                  (name, codecs, why)
    build(name, codec, N, C, rep=0, param=0, nobase=False) -> (x, base or None), fp16 arrays.  codec: "int8" / "int4" / "topk" (param = m).
    delta(x, base)         d = fp16(x - base), what the codec sees
    reps(name, N, C)       draws of a case that together put an extreme on every row position the case lists (extremes-placed: a 16-channel
                           tensor of 4098 rows has 32 extremes a draw and 266 positions)

A generator makes the residual d; _with_base then finds a base under it such that fp16(fp16(base + d) - base) is d BIT FOR BIT (the sign of a
zero included: -0 needs x = -0 over base = +0), trying an ordinary base first, then coarser and finer grids, then base = +0.  A generator that
needs particular base bits returns (x, base) itself."""
import zlib

import numpy as np

F16, F64 = np.float16, np.float64
U = 2.0 ** -24                    # fp16's smallest subnormal
NEG0 = np.uint16(0x8000)
MINMAX = ("int8", "int4")
TOPK_M = (1, 2, 4, 8, 16)
# the smallest shape that takes each launch form (tests/test_gpu_value_domain.py FORMS says which, and proves it by the kernel ids)
MINMAX_SHAPES = [(66, 144), (66, 528), (1026, 16), (2050, 16), (4098, 16), (66, 136), (18, 24), (1, 72), (2, 72)]
TOPK_SHAPES = [(128, 72), (16, 576), (128, 8)]
CROSS_PAIRS = [(3, 11), (7, 8), (0, 15), (8, 7), (15, 0)]     # (first listed, second listed) index of the planted pair in a 16-wide half-block


def delta(x, base):
    x = np.asarray(x).view(F16)
    if base is None:
        return x.copy()
    return (x.astype(F64) - np.asarray(base).view(F16).astype(F64)).astype(F16)


def _with_base(rng, d, strict=None):
    """(x, base) with fp16(x - base) == d bit for bit; where strict, x - base == d without any rounding"""
    d = np.ascontiguousarray(d, dtype=F16)
    want = d.view(np.uint16)
    base = np.zeros(d.shape, F16)
    todo = np.ones(d.shape, bool)
    cands = [rng.standard_normal(d.shape), rng.standard_normal(d.shape) * 2.0 ** -8, rng.integers(-128, 129, d.shape) * 32.0,
             rng.integers(-900, 901, d.shape) * U]
    with np.errstate(over="ignore", invalid="ignore"):
        for cand in cands:
            b = cand.astype(F16)
            x = (b.astype(F64) + d.astype(F64)).astype(F16)
            ok = np.isfinite(x) & ((x.astype(F64) - b.astype(F64)).astype(F16).view(np.uint16) == want)
            if strict is not None:
                ok &= ~strict | (x.astype(F64) - b.astype(F64) == d.astype(F64))
            take = todo & ok
            base[take] = b[take]
            todo &= ~ok
    x = (base.astype(F64) + d.astype(F64)).astype(F16)
    zero = (want & 0x7FFF) == 0
    x[todo & zero] = d[todo & zero]                 # (+0 + -0 is +0: a -0 residual is x = -0 over base = +0)
    assert (delta(x, base).view(np.uint16) == want).all() and np.isfinite(x).all()
    return x, base


# ---- int8 / int4 ----------------------------------------------------------------------------------------------------------------------
def extreme_rows(N):
    """row positions an extreme must visit: row 0, row N - 1, every residue mod 8 (every wave), both sides of every 32-row boundary (the
    64-row ones are among them)"""
    pos = {0, N - 1} | set(range(min(8, N)))
    for b in range(32, N, 32):
        pos |= {b - 1, b}
    return sorted(pos)


def reps(name, N, C):
    if name == "near-tie-quotients":
        return -(-len(_near()) // C)
    return -(-len(extreme_rows(N)) // (2 * (C - 2))) if name == "extremes-placed" else 1


def extreme_plan(N, C, rep):
    """(row of the minimum, row of the maximum) per channel: channel c of draw rep takes positions 2 * (c + rep * (C - 2)) and the next of
    the list, cyclically - and the LAST two channels (in the last active lane of a partial 512-channel block) take row N - 1 and row 0"""
    pos = extreme_rows(N)
    k = 2 * (np.arange(C) + rep * (C - 2))
    rmin, rmax = np.array(pos)[k % len(pos)], np.array(pos)[(k + 1) % len(pos)]
    if N > 1:
        rmin[C - 1], rmax[C - 1] = N - 1, 0
        rmin[C - 2], rmax[C - 2] = 0, N - 1
        clash = rmin == rmax
        rmax[clash] = (rmin[clash] + 1) % N
    return rmin, rmax


def _extremes_placed(rng, codec, N, C, rep):
    d = (rng.integers(-230, 231, (N, C)) / 256.0).astype(F16)                  # strictly inside +-0.9
    rmin, rmax = extreme_plan(N, C, rep)
    c = np.arange(C)
    d[rmax, c] = (1.0 + (c % 11) / 16.0).astype(F16)
    d[rmin, c] = (-1.0 - (c % 13) / 16.0).astype(F16)                          # (N == 1: the one row is both)
    return d


def _constant_channels(rng, codec, N, C, rep):
    d = rng.standard_normal((N, C)).astype(F16)
    if C > 512:                                       # a whole column block: constants that differ from channel to channel, zeros among them
        d[:, :512] = ((np.arange(512) % 9 - 4) / 8.0).astype(F16)[None, :]
    d[:, 0] = 0.0                                     # all +0
    d[:, 1] = 0.5                                     # all one non-zero value
    d[:, 2] = F16(3 * U)                              # range of one unit of 2^-24: the scale rounds to 0 under a non-zero range
    d[N // 2:, 2] = F16(4 * U)
    d[:, 3] = 0.0
    d[N - 1, 3] = F16(U)
    d[:, 4] = F16(-2 * U)
    d[0, 4] = F16(-3 * U)
    d[:, 5] = -1.75
    d[:, 8:16] = 0.25                                 # a whole lane of 8
    d[:, C - 1] = -0.5
    strict = np.zeros((N, C), bool)
    strict[:, 1] = True                               # x = base + 0.5 exactly
    return "d", d, strict


def zero_pairs(N):
    """(row of the -0, row of the +0) of a channel whose zero extreme has both signs: different waves of one tile (rows 1, 2), different
    32-row tiles (3, 40), the first and the last tile - each in both orders"""
    p = [(1, 2), (2, 1), (3, 40), (40, 3), (5, N - 2), (N - 2, 5), (0, N - 1), (N - 1, 0), (9, 14), (33, 36)]
    return [(a, b) for a, b in p if 0 <= a < N and 0 <= b < N and a != b]


def _signed_zero_extremes(rng, codec, N, C, rep):
    """channel c % 4: 0 = minimum zero with both signs (all d >= 0), 1 = maximum zero with both signs (all d <= 0), 2 = ordinary,
    3 = all zeros with both signs"""
    pairs = zero_pairs(N)
    mag = (rng.integers(1, 512, (N, C)) / 128.0).astype(F16)
    d = np.where(rng.integers(0, 2, (N, C)) == 1, mag, -mag).astype(F16)
    u = d.view(np.uint16)
    for c in range(C):
        kind = c % 4
        if kind == 2 or not pairs:
            continue
        a, b = pairs[(c // 4 + rep) % len(pairs)]
        if kind == 0:
            u[:, c] &= 0x7FFF
        elif kind == 1:
            u[:, c] |= 0x8000
        else:
            u[:, c] = np.where((np.arange(N) * 7 + c) % 3 == 0, NEG0, np.uint16(0))
        u[a, c], u[b, c] = NEG0, 0
    return d


def signed_zero_channels(name, N, C):
    """channels a case plants a both-signed zero MINIMUM in (the only ones the int4 packet's `min` half may differ on)"""
    if name == "signed-zero-extremes" and zero_pairs(N):
        return {c for c in range(C) if c % 4 in ((0, 1, 3) if N == 2 else (0, 3))}       # (two rows: the pair is the whole channel)
    return set()


def _offset(rng, codec, N, C, rep):
    hi = 100.0 + rng.integers(0, 17, (N, C)) / 16.0                            # [100, 101]: the int8 zero point saturates at -128
    lo = -2000.0 + rng.integers(0, 11, (N, C))                                 # [-2000, -1990]: ... at 127
    d = np.where((np.arange(C) % 2 == 0)[None, :], hi, lo).astype(F16)
    c = np.arange(C)
    d[0, c] = np.where(c % 2 == 0, 100.0, -2000.0).astype(F16)
    d[N - 1, c] = np.where(c % 2 == 0, 101.0, -1990.0).astype(F16)
    return d


def _tiny(rng, codec, N, C, rep):
    """whole units of 2^-24 in +-40: every scale is subnormal (int4: 0 .. 5 units).  An int8 scale of such a channel is 80 / 255 units: 0; so
    for int8 every other channel is in +-320 units instead (scales of 2 and 3 units)"""
    d = rng.integers(-40, 41, (N, C))
    if codec == "int8":
        d[:, 1::2] *= 8
    return (d * U).astype(F16)


def _wide(rng, codec, N, C, rep):
    d = rng.uniform(-28000.0, 28000.0, (N, C)).astype(F16)
    c = np.arange(C)
    d[(c * 5) % N, c] = (29000.0 + 16 * (c % 60)).astype(F16)                  # fp16(max - min) lies above 32768: a grid of 32
    d[(c * 5 + 1) % N, c] = (-29008.0 - 16 * (c % 57)).astype(F16)
    return d


def _range_overflow(rng, codec, N, C, rep):
    d = rng.standard_normal((N, C)).astype(F16)
    for k, c in enumerate((0, 5, 8, C - 1)):
        d[(3 * k) % N, c] = 60000.0
        d[(3 * k + 1 + (N - 1) // 2) % N, c] = -60000.0
    return d


def _rint_ties(rng, codec, N, C, rep):
    """scale exactly 1.0, every quotient between the extremes k + 1/2: int4 min 0 max 15; int8 min -100 max 155 (zero point -28)"""
    if codec == "int4":
        d = rng.integers(0, 15, (N, C)) + 0.5
        lo, hi = 0.0, 15.0
    else:
        d = rng.integers(0, 255, (N, C)) + 0.5 - 100.0
        lo, hi = -100.0, 155.0
    d = d.astype(F16)
    c = np.arange(C)
    d[(c * 3) % N, c] = hi
    d[(c * 3 + 1) % N, c] = lo
    return d


def near_tie_quotients():
    """int8 channels (R, [a ...]): minimum 0 and maximum R give the scale s = fp16(R / 255.000001) and the zero point -128; each a is an
    fp16 value whose quotient a / s lies within 2^-22 (relative) of the midpoint between the two fp16 values around k + 1/2 that rint sends
    to different codes.  An fp32 quotient that is off by a unit in its last place - a reciprocal multiplied in without the correcting
    step of hdiv_r - rounds to the other fp16 value there, and the code moves by one."""
    out = []
    k = np.arange(255.0)
    v = (k + 0.5).astype(F16)
    up, down = np.nextafter(v, F16(np.inf)).astype(F64), np.nextafter(v, F16(0)).astype(F64)
    M = np.where(k % 2 == 0, (v.astype(F64) + up) / 2, (v.astype(F64) + down) / 2)      # a tie goes to the even k; its far neighbour to k + 1
    for e in (0.0, -4.0, -9.0):
        for sig in range(1024, 2048):
            R = F16(sig / 1024.0 * 2.0 ** (7 + e))
            s = F64((np.float32(R) / np.float32(255.000001)).astype(F16))
            a0 = (M * s).astype(F16)
            cand = np.stack([np.nextafter(a0, F16(0)), a0, np.nextafter(a0, F16(np.inf))]).astype(F64)
            near = (np.abs(cand / s - M) < M * 2.0 ** -22) & (cand <= F64(R))
            if near.any():
                out.append((R, sorted(set(cand[near].tolist()))))
    return out


_NEAR = []


def _near():
    if not _NEAR:
        _NEAR.extend(near_tie_quotients())
    return _NEAR


def _near_ties(rng, codec, N, C, rep):
    d = np.zeros((N, C), F16)
    for c in range(C):
        R, a = _near()[(c + rep * C) % len(_near())]
        col = rng.uniform(0.0, float(R), N).astype(F16)
        col[(np.arange(len(a)) * 5 + 2 + c) % N] = a
        col[(c * 3) % N], col[(c * 3 + 1) % N] = 0.0, R
        d[:, c] = col
    return d


# ---- top-k: flat blocks of 1024, half-blocks of m ------------------------------------------------------------------------------------
def _tk_ties(rng, codec, N, C, rep, m):
    return (rng.integers(-3, 4, (N, C)) * 0.25).astype(F16)


def cross_plan(h):
    """half-block h of `cross-lane-ties`: (index a, index b, sign of a, sign of b, a third maximum inside the lower lane or -1)"""
    a, b = CROSS_PAIRS[h % 5]
    sa, sb = ((1, 1), (-1, -1), (1, -1), (-1, 1))[(h // 5) % 4]
    return a, b, sa, sb, (5 if (h // 20) % 3 == 2 and a == 3 else -1)


def _tk_cross_lane(rng, codec, N, C, rep, m):
    hb = (rng.integers(1, 64, (N * C // 16, 16)) / 128.0 * np.where(rng.integers(0, 2, (N * C // 16, 16)) == 1, 1, -1)).astype(F16)
    for h in range(hb.shape[0]):
        a, b, sa, sb, third = cross_plan(h + rep)
        hb[h, a], hb[h, b] = sa * 3.0, sb * 3.0
        if third >= 0:
            hb[h, third] = -3.0
    return hb.reshape(N, C)


def _tk_sweep(rng, codec, N, C, rep, m):
    hb = (rng.integers(-100, 101, (N * C // m, m)) / 128.0).astype(F16)
    h = np.arange(hb.shape[0])
    hb[h, (h + rep) % m] = np.where(h % 3 == 0, -2.0, 2.0).astype(F16)
    return hb.reshape(N, C)


def _tk_zero_half_blocks(rng, codec, N, C, rep, m):
    """every other half-block all zero with -0 at index 0 (and, every fourth, at its last index too); under the +0 elements that are not
    kept the BASE is -0 (x = +0): the state there is (-0) + (+0) = +0"""
    hb = rng.standard_normal((N * C // m, m)).astype(F16)
    z = np.arange(hb.shape[0]) % 2 == 0
    hb[z] = 0.0
    d = hb.view(np.uint16)
    d[z, 0] = NEG0
    d[z & (np.arange(hb.shape[0]) % 4 == 0), m - 1] = NEG0
    d = d.view(F16).reshape(N, C)
    x, base = _with_base(rng, d)
    plus0 = np.zeros((N * C // m, m), bool)
    plus0[z, 1:] = (hb.view(np.uint16)[z, 1:] == 0)
    plus0 = plus0.reshape(N, C)
    base.view(np.uint16)[plus0] = NEG0
    x.view(np.uint16)[plus0] = 0
    return x, base


def _tk_subnormal_and_max(rng, codec, N, C, rep, m):
    n = N * C // m
    hb = rng.standard_normal((n, m)).astype(F16)
    h = np.arange(n)
    sub = h % 3 == 0
    hb[sub] = (rng.integers(-1023, 1024, (n, m)) * U).astype(F16)[sub]          # subnormals only (zeros among them)
    big = h % 3 == 1
    hb[big, (h[big] // 3) % m] = np.where(h[big] % 2 == 0, 65504.0, -65504.0).astype(F16)
    two = big & (h % 4 == 1) & (m > 1)
    hb[two, (h[two] // 3 + m // 2) % m] = -65504.0                              # ... twice in a half-block: the first of the two is kept
    return hb.reshape(N, C)


# (name, codecs, why)
CASES = [
    ("extremes-placed", MINMAX, "every channel's minimum and maximum planted, everything else strictly inside; their rows rotate over row 0, "
     "row N - 1 (the ragged last tile), every residue mod 8 (every wave) and both sides of every 32- and 64-row boundary; channel C - 1 and "
     "the last active lane of a partial column block included"),
    ("constant-channels", MINMAX, "zero-range channels (all +0, all 0.5, a lane of 8, a whole column block where C > 512) and channels whose "
     "range is one unit of 2^-24: scale 0 under a non-zero range"),
    ("signed-zero-extremes", MINMAX, "channels with d >= 0 whose zero minimum occurs as -0 and as +0, in different waves of a tile and in "
     "different row tiles, both orders; the mirror image for the maximum; all-zero channels with both signs"),
    ("offset", MINMAX, "d in [100, 101] and in [-2000, -1990]: the int8 zero point saturates at -128 and at 127, the codes clamp"),
    ("tiny", MINMAX, "whole units of 2^-24 in +-40 (int8: every other channel +-320): subnormal scales, zero ones among them"),
    ("wide", MINMAX, "d over +-30000: fp16(max - min) finite, rounded on a 32-wide grid"),
    ("range-overflow", MINMAX, "+60000 and -60000 in one channel: max - min is infinite in fp16 (bit for bit against the oracle only)"),
    ("rint-ties", MINMAX, "scale exactly 1.0 and every quotient k + 1/2: every code a round-half-even tie"),
    ("near-tie-quotients", ("int8",), "int8 quotients within 2^-22 of the midpoint between the two fp16 values around a k + 1/2 that rint "
     "separates: the division has to be the correctly rounded one (hdiv_r's correcting step)"),
    ("ties", ("topk",), "d from the 7 multiples of 0.25 in +-0.75: every half-block ties, with both signs"),
    ("cross-lane-ties", ("topk",), "m = 16: the maximum twice in a half-block, at (3, 11), (7, 8), (0, 15), (8, 7), (15, 0), equal and opposite "
     "signs: both lanes of the vote decide a tie"),
    ("kept-index-sweep", ("topk",), "the single maximum at index 0 .. m - 1 in turn, half-blocks of flat blocks that straddle rows included"),
    ("zero-half-blocks", ("topk",), "all-zero half-blocks with -0 at index 0: the kept value is d[0] bit for bit; -0 base elements under "
     "elements that are not kept"),
    ("subnormal-and-max", ("topk",), "half-blocks of subnormals only, and |d| = 65504 (once and twice in a half-block)"),
]
_GEN = {"extremes-placed": _extremes_placed, "constant-channels": _constant_channels, "signed-zero-extremes": _signed_zero_extremes,
        "offset": _offset, "tiny": _tiny, "near-tie-quotients": _near_ties, "wide": _wide, "range-overflow": _range_overflow, "rint-ties": _rint_ties, "ties": _tk_ties,
        "cross-lane-ties": _tk_cross_lane, "kept-index-sweep": _tk_sweep, "zero-half-blocks": _tk_zero_half_blocks,
        "subnormal-and-max": _tk_subnormal_and_max}
FINITE = {n for n, _, _ in CASES} - {"range-overflow"}        # the float64 definition applies


def applies(name, codec, N, C, param=0):
    """the case can be built at this shape for this codec"""
    codecs = dict((n, c) for n, c, _ in CASES)[name]
    if codec not in codecs:
        return False
    if name == "cross-lane-ties":
        return param == 16
    if name in ("signed-zero-extremes", "range-overflow"):
        return N >= 2
    if name == "near-tie-quotients":
        return N >= 16
    return True


def legal(codec, N, C, param=0):
    if codec == "topk":
        return (N * C) % 1024 == 0 and C % 8 == 0
    return C % 8 == 0 and N >= 1 and (codec == "int8" or N % 2 == 0)


def shapes_for(codec):
    return [s for s in (TOPK_SHAPES if codec == "topk" else MINMAX_SHAPES) if legal(codec, *s)]


def cases_for(codec, N, C, param=0):
    return [n for n, _, _ in CASES if applies(n, codec, N, C, param)]


def build(name, codec, N, C, rep=0, param=0, nobase=False):
    """(x, base or None) of a case: the same arrays on every call (rep: another draw of the same case)"""
    assert applies(name, codec, N, C, param), (name, codec, N, C, param)
    tag = f"{name}-{codec if name in ('rint-ties', 'tiny') else codec[:3]}-{N}-{C}-{rep}-{param}"
    rng = np.random.default_rng(zlib.crc32(tag.encode()))
    out = _GEN[name](rng, codec, N, C, rep, param) if codec == "topk" else _GEN[name](rng, codec, N, C, rep)
    strict = None
    if isinstance(out, tuple) and isinstance(out[0], str):
        _, out, strict = out
    if isinstance(out, tuple):
        x, base = out
        return (delta(x, base), None) if nobase else (x, base)
    d = np.ascontiguousarray(out, dtype=F16).reshape(N, C)
    assert np.isfinite(d).all()
    return (d, None) if nobase else _with_base(rng, d, strict)
