"""The shape and VALUE domain of the INT2_MINMAX codec (levels 0 .. 3, four rows per code byte) as deterministic cases, in the manner of
tests/_value_cases.py, whose generators are used wherever they do not depend on the number of levels.  Shared by
tests/test_int2mm_contract.py (CPU: the numpy contract against the float64 definition, and the proof that each case holds what its `why`
says) and tests/test_gpu_int2mm.py (GPU: every launch form against the contract).

    SHAPES                 the smallest shapes that reach each mechanism (N a multiple of 4)
    CASES                  (name, why)
    build(name, N, C, rep=0, nobase=False) -> (x, base or None) fp16 arrays ; reps(name, N, C)
"""
import zlib

import numpy as np

import _value_cases as V

F16, F64 = np.float16, np.float64
U = V.U

SHAPES = {
    "one quad, tails not 16-byte aligned": [(4, 72), (8, 72)],
    "C off the 512-channel tile": [(20, 24), (68, 136), (68, 144), (68, 528), (132, 520), (4, 1168)],
    "tile heights 32 / 64, row tiles not filled": [(132, 144), (516, 192), (544, 576)],
    "more than 64 partials per channel": [(1028, 16), (2052, 16), (4100, 16)],
}
ALL_SHAPES = [s for v in SHAPES.values() for s in v]


def extreme_rows(N):
    """row positions an extreme must visit: every row class of a quad and of a tile - every row of the first 64 (each wave's quad of a
    32-row tile and of a 64-row tile, every position in the quad), row N - 1 and the last quad, both sides of every 32-row boundary"""
    pos = set(range(min(64, N))) | set(range(max(0, N - 4), N))
    for b in range(32, N, 32):
        pos |= {b - 1, b}
    return sorted(pos)


def reps(name, N, C):
    return -(-len(extreme_rows(N)) // (2 * (C - 2))) if name == "extremes-placed" else 1


def extreme_plan(N, C, rep):
    pos = np.array(extreme_rows(N))
    k = 2 * (np.arange(C) + rep * (C - 2))
    rmin, rmax = pos[k % len(pos)], pos[(k + 1) % len(pos)]
    rmin[C - 1], rmax[C - 1] = N - 1, 0
    rmin[C - 2], rmax[C - 2] = 0, N - 1
    clash = rmin == rmax
    rmax[clash] = (rmin[clash] + 1) % N
    return rmin, rmax


def _extremes_placed(rng, N, C, rep):
    d = (rng.integers(-230, 231, (N, C)) / 256.0).astype(F16)
    rmin, rmax = extreme_plan(N, C, rep)
    c = np.arange(C)
    d[rmax, c] = (1.0 + (c % 11) / 16.0).astype(F16)
    d[rmin, c] = (-1.0 - (c % 13) / 16.0).astype(F16)
    return d


def tie_values():
    """scale exactly 1.0 (min 0, max 3): the quotient IS d.  0.5 / 1.5 / 2.5 (ties: codes 0, 2, 2) and the fp16 neighbour on either side"""
    out = []
    for t in (0.5, 1.5, 2.5):
        v = F16(t)
        out += [np.nextafter(v, F16(0)), v, np.nextafter(v, F16(4))]
    return np.array(out, F16)


def _rint_ties(rng, N, C, rep):
    d = tie_values()[rng.integers(0, 9, (N, C))]
    c = np.arange(C)
    d[(c * 3) % N, c] = 3.0
    d[(c * 3 + 1) % N, c] = 0.0
    return d


def _clamp_at_top(rng, N, C, rep):
    """whole units of 2^-24 in 0 .. k, k = 1 + c % 12: the subnormal scale fp16(k / 3.000001 units) is rounded to a whole unit - down for
    k = 4 (1.33 -> 1: the maximum's quotient is 4, it clamps at 3), 7, 10 ...; k = 1: scale 0, +inf quotients clamp at 3"""
    c = np.arange(C)
    k = 1 + c % 12
    d = rng.integers(0, 1 << 30, (N, C)) % (k + 1)[None, :]
    d[(c * 3) % N, c] = k
    d[(c * 3 + 1) % N, c] = 0
    return (d * U).astype(F16)


# the generators of tests/_value_cases.py that do not depend on the number of levels take "int4"
def _from_v(name):
    return lambda rng, N, C, rep: V._GEN[name](rng, "int4", N, C, rep)


CASES = [
    ("extremes-placed", "every channel's minimum and maximum planted, everything else strictly inside; their rows rotate over every row of "
     "the first two 32-row tiles (every wave's quad, every position in it), the last quad, both sides of every 32-row boundary"),
    ("constant-channels", "zero-range channels (scale 0, NaN quotient: code 0, reconstruction = min) and channels whose range is one unit "
     "of 2^-24 (scale 0 under a non-zero range: +inf quotients clamp at 3)"),
    ("signed-zero-extremes", "zero minima / maxima occurring as -0 and as +0, in different waves and row tiles, both orders"),
    ("tiny", "whole units of 2^-24 in +-40: subnormal scales"),
    ("clamp-at-top", "ranges of 1 .. 12 units of 2^-24: scales rounded down to a whole unit put the maximum's quotient above 3.5"),
    ("wide", "d over +-30000: fp16(max - min) finite, rounded on a 32-wide grid"),
    ("range-overflow", "+60000 and -60000 in one channel: max - min is infinite in fp16 (against the contract only, not float64)"),
    ("rint-ties", "scale exactly 1.0; quotients exactly 0.5 / 1.5 / 2.5 (round half to even) and one fp16 ulp on either side"),
]
_GEN = {"extremes-placed": _extremes_placed, "rint-ties": _rint_ties, "clamp-at-top": _clamp_at_top}
for _n in ("constant-channels", "signed-zero-extremes", "tiny", "wide", "range-overflow"):
    _GEN[_n] = _from_v(_n)
NAMES = [n for n, _ in CASES]
FINITE = set(NAMES) - {"range-overflow"}


def signed_zero_channels(name, N, C):
    return V.signed_zero_channels(name, N, C)


def build(name, N, C, rep=0, nobase=False):
    """(x, base or None) of a case: the same arrays on every call"""
    assert N % 4 == 0 and C % 8 == 0
    rng = np.random.default_rng(zlib.crc32(f"i2mm-{name}-{N}-{C}-{rep}".encode()))
    out = _GEN[name](rng, N, C, rep)
    strict = None
    if isinstance(out, tuple) and isinstance(out[0], str):
        _, out, strict = out
    d = np.ascontiguousarray(out, dtype=F16).reshape(N, C)
    assert np.isfinite(d).all()
    return (d, None) if nobase else V._with_base(rng, d, strict)
