"""The VALUE domain of the bf16 exchange (1-bit and 2-bit codecs with CFX_ELEM_BF16), as deterministic cases - a plain module like
tests/_domain_cases.py (which holds the shapes), shared by tests/test_bf16_domain_f64.py (CPU: the contract against the definition, and
the proof that every kind of case is present) and tests/test_gpu_bf16_domain.py (GPU: the kernels against the contract and the
definition).  bf16 tensors are uint16 bit patterns.  Every case stays inside the documented domain: finite values, |x - base| < 65504.

    CASES            (name, shapes, why); build(name, N, C) -> (x, base or None)
    TIE_SHAPES       hand-built packets whose reconstruction lands exactly halfway between two bf16 values:
                     tie_packet(name, N, C) -> (base, packet words); tie_quantize(N, C) -> (x, base, tok, chan) for cfx_int2_quantize

Shapes: LAYER takes the one-launch layer form (C % 128 == 0; it is the FLUX U = 8 K,V shard), the others do not (C % 128 != 0), or are
the second shape of tests/test_gpu_parity.py's drift tests."""
import zlib

import numpy as np
import torch

LAYER = (544, 3072)
PIXART = (544, 576)
SMALL = (129, 144)
TALL = (130, 1024)
U2 = 2.0 ** -24                   # fp16's smallest subnormal: the unit of the kernels' exact sums


def bf16_bits(a32):
    """float32 array -> bf16 bits (nearest even)"""
    t = torch.from_numpy(np.ascontiguousarray(a32, dtype=np.float32)).to(torch.bfloat16)
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def bf16_f32(u16):
    return (np.ascontiguousarray(u16).astype(np.uint32) << 16).view(np.float32)


def _exact(a):
    """values that ARE bf16 values -> their bits"""
    a = np.asarray(a, dtype=np.float32)
    u = a.view(np.uint32)
    assert not (u & 0xFFFF).any(), "not a bf16 value"
    return (u >> 16).astype(np.uint16)


def _ordinary(rng, N, C, drift=0.2, scale=0.5):
    base = bf16_bits(scale * rng.standard_normal((N, C)))
    x = bf16_bits(bf16_f32(base) + drift * rng.standard_normal((N, C)).astype(np.float32))
    return x, base


def _large(rng, N, C):
    e = rng.integers(10, 23, (N, C))
    m = rng.integers(0, 128, (N, C))
    s = rng.integers(0, 2, (N, C))
    base = ((s << 15) | ((e + 127) << 7) | m).astype(np.uint16)
    k = rng.integers(-3, 4, (N, C))
    k = np.where(e >= 21, np.clip(k, -1, 1), k)           # (3 ulp of 2^14 or 2^15, across a binade, would leave the fp16 range)
    x = (base.astype(np.int64) + k).astype(np.uint16)     # sign-magnitude: the magnitude moves by k bf16 ulp; k == 0: x == base
    return x, base


def _tiny(rng, N, C):
    x, base = _ordinary(rng, N, C)

    def bits(rows, lo, hi):
        shp = (rows, C)
        return ((rng.integers(0, 2, shp) << 15) | (rng.integers(lo, hi, shp) << 7) | rng.integers(0, 128, shp)).astype(np.uint16)

    def sub(rows):
        return ((rng.integers(0, 2, (rows, C)) << 15) | rng.integers(1, 128, (rows, C))).astype(np.uint16)

    def sgn(rows):
        return np.where(rng.integers(0, 2, (rows, C)) == 1, np.float32(-1), np.float32(1))
    x[0:2], base[0:2] = bits(2, 27, 97), bits(2, 27, 97)          # normals 2^-100 .. 2^-31: d underflows to +-0
    x[2:4], base[2:4] = sub(2), sub(2)                            # bf16 subnormals on both sides
    for r in (4, 5):                                              # a subnormal against an ordinary value (kept above 2^-10: a bf16 value
        for t in (x, base):                                       # of 8 bits is then an fp16 value, whatever the subnormal adds)
            v = bf16_f32(t[r])
            t[r] = bf16_bits(np.where(np.abs(v) < 2.0 ** -10, np.float32(2.0 ** -10), v))
    x[4], base[5] = sub(1)[0], sub(1)[0]
    a, b = rng.integers(0, 256, (4, C)), rng.integers(0, 256, (4, C))
    x[6:10] = _exact(sgn(4) * a.astype(np.float32) * np.float32(U2))        # whole units of 2^-24: d inside fp16's subnormal range, exact
    base[6:10] = _exact(sgn(4) * b.astype(np.float32) * np.float32(U2))
    a = rng.integers(0, 128, (2, C))
    x[10:12] = _exact(sgn(2) * (2 * a + 1).astype(np.float32) * np.float32(U2 / 2))     # half units: d is a TIE of the subnormal grid
    base[10:12] = _exact(sgn(2) * rng.integers(0, 128, (2, C)).astype(np.float32) * np.float32(U2))
    return x, base


NEG0 = np.uint16(0x8000)


def _signed_zeros(rng, N, C):
    x, base = _ordinary(rng, N, C)
    x[0], base[0] = 0, 0                          # +0 - +0
    x[1], base[1] = NEG0, 0                       # -0 - +0 = -0: its sign bit must pack as d >= 0
    x[2], base[2] = 0, NEG0
    x[3], base[3] = NEG0, NEG0
    x[4:, 8:16:2], base[4:, 8:16:2] = NEG0, 0     # columns of zero residual with both zeros
    x[4:, 9:16:2], base[4:, 9:16:2] = NEG0, NEG0
    x[6:40, 40::7] = NEG0                         # scattered: x a zero against an ordinary base, and the reverse
    base[41:80, 41::5] = NEG0
    return x, base


def _signed_zeros_no_base(rng, N, C):
    """base None: the state is bf16(recv), and recv is -0 where the sign bit is 0 under a scale that rounds to 0 - a column whose only
    non-zero element is -2^-24 (mean 2^-24 / N: fp16 0).  fp32(+0) + fp32(-0) would be +0: el_state's has_base branch."""
    x, _ = _ordinary(rng, N, C)
    x[:, 0:8] = 0
    x[:, 1] = NEG0
    x[5, 0] = x[7, 2] = x[N - 1, 7] = _exact(np.float32(-U2))
    x[5, 3] = _exact(np.float32(U2))
    x[9, :] = np.where(np.arange(C) % 2 == 0, NEG0, np.uint16(0))         # a row of zeros
    return x, None


def _zero_rows_cols(rng, N, C):
    x, base = _ordinary(rng, N, C)
    base[1, 0:8] = (np.arange(8) + 1).astype(np.uint16)                 # subnormal states under a zero residual: base + (+-0) keeps them
    base[2:N:3, C - 1] = (np.arange(len(range(2, N, 3))) % 127 + 1).astype(np.uint16) | NEG0
    for r in (1, 33, N - 1):
        x[r] = base[r]
    for c in (0, 9, C - 1):
        x[:, c] = base[:, c]
    x[:, 16:24] = base[:, 16:24]                                        # a whole lane of 8 channels
    return x, base


def _drift(d):
    def gen(rng, N, C):
        base = bf16_bits(rng.standard_normal((N, C)))                   # base of order 1: x - base stays far inside +-65504 at drift 3000
        x = bf16_bits(bf16_f32(base) + np.float32(d) * rng.standard_normal((N, C)).astype(np.float32))
        return x, base
    return gen


def _near_max(rng, N, C):
    x, base = _ordinary(rng, N, C, drift=0.1)

    def put(r, c, xv, bv):
        x[r, c], base[r, c] = _exact(np.float32(xv)), _exact(np.float32(bv))
    put(5, 17, 59904.0, -96.0)                    # d = +60000
    put(5, 18, -59904.0, 96.0)                    # d = -60000, the same row
    put(7, 3, 65280.0, -192.0)                    # d = 65472, the largest fp16 below 65504
    put(N - 1, C - 1, -65280.0, 208.0)            # d = -65488: halfway between -65472 and -65504, to even: -65472
    put(9, 40, 65280.0, -223.0)                   # d = 65503 -> fp16 65504
    put(11, 5, -65280.0, 223.0)
    return x, base


# (name, shapes, why)
CASES = [
    ("large", [LAYER, SMALL], "|x|, |base| up to 2^22 - beyond fp16 - with x 0 .. 3 bf16 ulp from base (x == base included: d = +0): the "
     "subtraction must be the fp32 one, and the state's rounding works on 2^15-sized ulps"),
    ("tiny", [LAYER, PIXART, SMALL], "normals below 2^-30 (d underflows to +-0), bf16 subnormals as x and base (fp32 subnormals once widened), "
     "differences inside fp16's subnormal range, whole units and ties"),
    ("signed-zeros", [LAYER, SMALL], "+-0 in x and in base, rows and columns of them: -0 - +0 = -0 packs as d >= 0"),
    ("signed-zeros-no-base", [LAYER, SMALL], "base None: a -0 received value must stay -0 in the state (el_state's has_base branch)"),
    ("zero-rows-cols", [LAYER, PIXART, SMALL], "whole rows and whole columns of zero residual (U[n] = 0, V[c] = 0; never the whole tensor: "
     "0 / 0 is outside the contract), subnormal states under them"),
    ("drift-1.5", [LAYER, TALL], "row partials of a 512-channel block beyond the 32-bit hand-over words (2^32 units of 2^-24 = 256)"),
    ("drift-50", [LAYER, TALL], "every row and column partial beyond the 32-bit words"),
    ("drift-400", [LAYER, TALL], "row partials beyond the 40-bit tagged words of the layer launches (2^40 units = 65536)"),
    ("drift-3000", [LAYER, TALL], "column partials of a 32-row tile beyond the 40-bit tagged words too"),
    ("near-max", [LAYER, PIXART, SMALL], "a row holding d = +60000 and -60000, |d| = 65472 / 65488 (a tie) / 65503 elsewhere"),
]
_GEN = {"large": _large, "tiny": _tiny, "signed-zeros": _signed_zeros, "signed-zeros-no-base": _signed_zeros_no_base,
        "zero-rows-cols": _zero_rows_cols, "drift-1.5": _drift(1.5), "drift-50": _drift(50.0), "drift-400": _drift(400.0),
        "drift-3000": _drift(3000.0), "near-max": _near_max}
DRIFTS = [n for n, _, _ in CASES if n.startswith("drift")]


def build(name, N, C, rep=0):
    """(x, base or None) of a case: the same arrays on every call (rep: another draw of the same case)"""
    rng = np.random.default_rng(zlib.crc32(f"{name}-{N}-{C}-{rep}".encode()))
    return _GEN[name](rng, N, C)


def all_cases():
    return [(n, N, C) for n, shapes, _ in CASES for N, C in shapes]


# ---- round-to-even ties in the state --------------------------------------------------------------------------------------------------
TIE_SHAPES = [LAYER, SMALL]


def _tie_base(rng, N, C):
    """base[n, c] = +-(1 + m/128) * 2^e[c], m in 4 .. 120 (both parities of the bf16 significand; no binade is crossed by +- 2.5 ulp);
    returns (bits, e) - one bf16 ulp of column c is 2^(e[c] - 7)"""
    e = rng.integers(-4, 5, C)
    m = rng.integers(4, 121, (N, C))
    s = rng.integers(0, 2, (N, C))
    return ((s << 15) | ((e[None, :] + 127) << 7) | m).astype(np.uint16), e


def tie_packet(name, N, C):
    """(base, packet words): row scales 1.0, column scales chosen so that fp32(base) + fp32(recv) is base +- (j + 1/2) bf16 ulp, j in
    0 .. 2 - exactly halfway between two bf16 values, the lower one even or odd as m + j falls - with random sign bits.  1-bit: recv =
    +-V[c], V[c] = (2j + 1) * 2^(e - 8).  2-bit: recv = +-0.5 chan (magnitude bit 0) or +-2 chan (bit 1); even columns take chan =
    (2j + 1) * 2^(e - 7), whose 0.5-level is the tie, odd columns chan = (2j + 1) * 2^(e - 9), whose 2.0-level is.  Columns 0 .. 7 carry
    scale 0 instead: recv = +-0 (with base None the state is then the signed zero itself)."""
    rng = np.random.default_rng(zlib.crc32(f"tie-{name}-{N}-{C}".encode()))
    base, e = _tie_base(rng, N, C)
    j = rng.integers(0, 3, C)
    if name == "binary":
        col = (2 * j + 1) * np.exp2(e - 8.0)
        codes = rng.integers(0, 256, N * C // 8, dtype=np.uint8)
    else:
        col = (2 * j + 1) * np.exp2(np.where(np.arange(C) % 2 == 0, e - 7.0, e - 9.0))
        codes = rng.integers(0, 256, N * C // 4, dtype=np.uint8)
    col[0:8] = 0.0
    col16 = col.astype(np.float16)
    assert (col16.astype(np.float64) == col).all()
    pkt = np.concatenate([codes, np.ones(N, np.float16).view(np.uint8), col16.view(np.uint8)])
    return base, pkt.view(np.uint16)


def tie_quantize(N, C):
    """(x, base, tok, chan) for cfx_int2_quantize with planted scales: the tie scales of tie_packet("int2"), x a few bf16 ulp from base so
    that both magnitude bits occur"""
    rng = np.random.default_rng(zlib.crc32(f"tieq-{N}-{C}".encode()))
    base, e = _tie_base(rng, N, C)
    j = rng.integers(0, 3, C)
    chan = ((2 * j + 1) * np.exp2(np.where(np.arange(C) % 2 == 0, e - 7.0, e - 9.0))).astype(np.float16)
    x = (base.astype(np.int64) + rng.integers(-3, 4, (N, C))).astype(np.uint16)
    return x, base, np.ones(N, np.float16), chan
