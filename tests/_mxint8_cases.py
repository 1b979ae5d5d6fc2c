"""Deterministic inputs of the MXINT8 suites (tests/test_mxint8_contract.py on the CPU, tests/test_gpu_mxint8.py on the GPU): the shapes at
which the kernels can go wrong and the value cases of the contract (include/cfx.h, "MXINT8").  A case plants whole blocks of 32 deltas: on a
planted block the state is +0, so that x - base is the planted value bit for bit (-0 - +0 = -0); everywhere else x and base are random with
block-wise magnitudes.  All tensors are uint16 bit patterns, fp16 or bf16.  For bf16 a planted finite fp16 delta v is split into x = the top
8 significant bits of v and base = -(the rest), both bf16 values whose fp32 difference is v exactly (tests/_bblock_cases.py; base None: x
alone), a NaN or an inf is x itself; the case "bf16" is built in bf16 directly.  A tensor with fewer blocks than a case has planted blocks
takes them over `reps(case, N, C)` repetitions."""
import numpy as np

import _bblock_cases as BK

F16, F32 = np.float16, np.float32
BLOCK = 32
# (1, 64): the 16-bit scale tail store alone; (1, 128): one full 32-bit scale store; (3, 192): E % 128 == 64 behind full words; (5, 320): a
# partial last wave; (4, 2112): one element past an S workgroup's 8192 elements with E % 2048 != 0; (129, 128): one unit past a D workgroup's
# 16384 elements
SHAPES = [(1, 64), (1, 128), (3, 192), (5, 320), (4, 2112), (129, 128)]
LAYER16 = (544, 3072)            # once per element type: the 16-item layer (the FLUX shard)
X_ALL = list(range(-18, 16))


def _h(bits):
    return np.asarray(bits, dtype=np.uint16).view(F16)


def _f16(vals):
    """float64 values that must be fp16 values"""
    v = np.asarray(vals, dtype=np.float64)
    h = v.astype(F16)
    assert np.array_equal(h.astype(np.float64), v), "not an fp16 value"
    return h


def _fill(vals, rng, small_bits):
    """a block of 32: `vals` first (fp16), the rest random of either sign with magnitude bits at most `small_bits` (None: zeros)"""
    v = np.zeros(BLOCK, dtype=F16)
    vals = np.asarray(vals, dtype=F16).reshape(-1)
    assert vals.size <= BLOCK
    v[:vals.size] = vals
    n = BLOCK - vals.size
    if small_bits is not None and n:
        v[vals.size:] = _h(rng.integers(0, int(small_bits) + 1, n).astype(np.uint16) | (rng.integers(0, 2, n).astype(np.uint16) << 15))
    return v


def _top(X):
    """fp16 bits of 2^X (X >= -24)"""
    return ((X + 15) << 10) if X >= -14 else (1 << (X + 24))


def _blocks(case, rng):
    """the planted blocks of a case: a list of 32-vectors of fp16 deltas"""
    out = []
    if case == "zeros":
        out.append(np.zeros(BLOCK, dtype=F16))
        out.append(_h(np.full(BLOCK, 0x8000)))                                   # a block of -0
        out.append(_h(np.where(np.arange(BLOCK) % 2, 0x8000, 0)))
        for X in (-18, -3, 15):                                                  # -0 elements, and negative deltas that round to 0, among non-zeros
            m = np.ldexp(1.0, X)
            small = [-m / 256, m / 256, -m / 128] if X - 7 >= -24 else []       # |y| = 0.25, 0.25, 0.5 (the tie to 0)
            out.append(_fill(np.concatenate([_f16([m, -m] + small), _h([0x8000, 0x8000, 0, 0x8000])]), rng, None))
    elif case == "every-X":
        # block maxima at 2^e (X = e), one ulp below (X = e - 1: the last value of the binade below, saturating to 127 there) - so every
        # X from -18 to 15 at its lowest and its highest maximum, and everything below the clamp
        for e in range(-24, 16):
            b = _top(e)
            for a in ((b, b - 1) if b > 1 else (b,)):
                for sign in (0, 0x8000):
                    out.append(_fill(_h([a | sign, (a | sign) ^ 0x8000]), rng, a))
        out.append(_fill(_h([0x7BFF, 0xFBFF]), rng, 0x7BFF))                   # 2^16 minus one ulp
    elif case == "ties":
        # y = k + 0.5 for even and odd k, both signs: rounds to the even neighbour
        for X in (-17, -16, -12, -1, 0, 9, 15):
            step = np.ldexp(1.0, X - 6)
            ks = [0, 1, 2, 3, 4, 5, 30, 31, 62, 63, 64, 65, 100, 101, 125, 126]
            vals = [np.ldexp(1.0, X)] + [s * (k + 0.5) * step for k in ks[:8] for s in (1.0, -1.0)]
            out.append(_fill(_f16(vals), rng, None))
            near = [0.25 * step, -0.75 * step, 1.25 * step, -1.75 * step] if X >= -14 else []      # (beside the ties: not ties)
            vals = [-np.ldexp(1.0, X)] + [s * (k + 0.5) * step for k in ks[8:] for s in (1.0, -1.0)] + near
            out.append(_fill(_f16(vals), rng, None))
    elif case == "saturation":
        # y in [127.5, 128) and exactly 127.5 saturate to 127 (the top 1/128 of a binade); 127.4375 and 126.5 (the tie, to 126) do not
        for X in (-16, -15, -14, -8, 0, 7, 14, 15):
            step = np.ldexp(1.0, X - 6)
            sh = X + 18
            fr = [127.5, 127.5 + 1 / 16, 127.75, 128 - 1 / 16, 127.4375, 127.0, 126.5, 126.5 + 1 / 16] if X >= -14 else \
                 [127.5, 127.0, 126.5] + ([127.75, 127.25] if sh >= 2 else [])
            vals = [s * y * step for y in fr for s in (1.0, -1.0)]
            out.append(_fill(_f16(vals), rng, _top(X) if X > -24 else 0))
    elif case == "max-65504":
        out.append(_fill(_f16([65504, -65504, 65024, -65024, 65280, 512, -256, 768]), rng, 0x7BFF))     # X = 15, q = +-127, recv +-65024
        out.append(_fill(_f16([-65504, 1, 2, 3]), rng, 0x6800))
        out.append(np.full(BLOCK, 65504, dtype=F16))
        out.append((np.where(np.arange(BLOCK) % 3 == 0, -1, 1) * 65504.0).astype(F16))
    elif case == "lossless":
        # below 2^-17 the block is reproduced exactly (128 units): below the clamp (max < 64 units) and on its boundary [2^-18, 2^-17)
        for top in (1, 2, 3, 31, 63, 64, 65, 100, 126, 127):
            for sign in (0, 0x8000):
                v = rng.integers(0, top + 1, BLOCK).astype(np.uint16) | (rng.integers(0, 2, BLOCK).astype(np.uint16) << 15)
                v[rng.integers(0, BLOCK)] = top | sign
                out.append(_h(v))
        out.append(_h(np.arange(BLOCK) * 4 + 3))                                 # every residue, max 127 units
        out.append(_h((np.arange(BLOCK) * 4 + 1) | 0x8000))
        for top in (128, 129, 255):                                              # the first blocks that are NOT exact: steps of 2 units
            out.append(_h(np.concatenate([[top], np.arange(1, BLOCK) | ((np.arange(1, BLOCK) % 2) << 15)]).astype(np.uint16)))
    elif case == "max-position":
        for pos in range(BLOCK):                                                 # each of the 4 lanes, each of a lane's 8 slots
            v = _fill([], rng, 0x3C00)
            v[pos] = F16(-48.0 if pos % 2 else 48.0)
            out.append(v)
    elif case == "nonfinite":
        out.append(_fill([1.0, np.nan, np.inf, -3.0], rng, 0x4800))
        out.append(_fill([-np.inf, 2.0], rng, 0x4000))
        out.append(_fill([np.inf], rng, 0x4000))
        out.append(_fill([np.nan], rng, 0x4000))
        v = _fill([], rng, 0x4000)
        v[BLOCK - 1] = np.nan
        out.append(v)
    else:
        assert case in ("random", "neighbours", "bf16"), case
    return out


NAMES = ["random", "zeros", "every-X", "ties", "saturation", "max-65504", "lossless", "neighbours", "max-position", "nonfinite", "bf16"]
NONFINITE = ("nonfinite", "bf16")          # cases with 0xFF blocks (bf16: differences that overflow fp16)
N_BF16_SPECIAL = 5


def cases_for(bf16):
    return NAMES if bf16 else [c for c in NAMES if c != "bf16"]


def n_planted(case):
    return N_BF16_SPECIAL if case == "bf16" else len(_blocks(case, np.random.default_rng(0)))


def reps(case, N, C):
    """repetitions a tensor of this shape needs to carry every planted block of the case"""
    return max(1, -(-n_planted(case) // (N * C // BLOCK)))


def _to_bf16_pair(v16):
    """planted fp16 deltas -> bf16 bits (x, base): fp32(x) - fp32(base) == v exactly; a NaN or an inf is x itself, base +0"""
    v16 = np.ascontiguousarray(v16, dtype=F16)
    fin = np.isfinite(v16)
    sx, sb = BK._split_bf16(np.where(fin, v16, F16(0)))
    raw = (v16.astype(F32).view(np.uint32) >> 16).astype(np.uint16)             # inf: 0x7f80 / 0xff80, NaN: 0x7fc0
    return np.where(fin, sx, raw), np.where(fin, sb, np.uint16(0))


def _bf16_special(rng):
    """(x, base) fp32 blocks of bf16 values: differences that overflow fp16, and round-to-even ties of the bf16 state"""
    sp = []
    # x - base = 2^18 and -2^18 among small differences, and 65536 = the first value that rounds to inf: the 0xFF block
    b = np.ldexp(rng.integers(128, 256, BLOCK).astype(np.float64), 10) * np.where(rng.integers(0, 2, BLOCK), -1.0, 1.0)
    x = b.copy()
    x[3], b[3] = np.ldexp(1.0, 17), -np.ldexp(1.0, 17)
    x[17], b[17] = -np.ldexp(1.0, 17), np.ldexp(1.0, 17)
    sp.append((x, b))
    x, b = np.ldexp(rng.integers(128, 256, BLOCK).astype(np.float64), -7), np.zeros(BLOCK)
    x[31], b[31] = 65280.0, -256.0                                               # 65536 exactly
    sp.append((x, b))
    # ties: base = 1 or 3 half-ulps of binade P, x = (128 + 2j) 2^(P-7): d = x - base is an fp16 value, y = 64 + j - 0.25 / 0.75, so recv
    # = q 2^(P-6) has an even bf16 significand and base + recv lies half-way between two bf16 values - below an even one (base one
    # half-ulp: stays) or an odd one (three: goes up)
    for P in (0, 5, -9):
        j = np.arange(BLOCK)
        x = (128 + 2 * j).astype(np.float64) * np.ldexp(1.0, P - 7)
        b = np.where(j % 2, 3.0, 1.0) * np.ldexp(1.0, P - 8)
        s = np.where(j % 8 < 4, 1.0, -1.0)
        sp.append((x * s, b * s))
    assert len(sp) == N_BF16_SPECIAL
    return sp


def build(case, N, C, bf16=False, rep=0, nobase=False, seed=0):
    """-> (x, base | None): uint16 bit patterns (N, C), fp16 or bf16"""
    assert C % 64 == 0 and (bf16 or case != "bf16")
    rng = np.random.default_rng([NAMES.index(case), N, C, rep, seed, int(bf16)])
    NB, CB = N * C // BLOCK, C // BLOCK
    if case == "bf16":
        # states far beyond fp16 whose difference is small (tests/_bblock_cases.py), then this codec's own blocks
        x, base = BK._bf16_direct(N, C, BLOCK, rng, rep)
        x, base = x.reshape(NB, BLOCK).copy(), base.reshape(NB, BLOCK).copy()
        sp = _bf16_special(rng)
        take = sp[rep * NB:(rep + 1) * NB] if len(sp) > NB else sp
        for p, (sx, sb) in zip(BK._positions(len(take), NB), take):
            x[p], base[p] = BK._f32_to_bf16(sx.astype(F32)), BK._f32_to_bf16(sb.astype(F32))
            assert np.array_equal((x[p].astype(np.uint32) << 16).view(F32), sx) and np.array_equal((base[p].astype(np.uint32) << 16).view(F32), sb)
        x, base = np.ascontiguousarray(x.reshape(N, C)), np.ascontiguousarray(base.reshape(N, C))
        if nobase:                                               # the differences themselves, cut to bf16: small values with no state
            with np.errstate(over="ignore", invalid="ignore"):
                d = (x.astype(np.uint32) << 16).view(F32) - (base.astype(np.uint32) << 16).view(F32)
            return np.ascontiguousarray((d.view(np.uint32) >> 16).astype(np.uint16)), None
        return x, base
    mag = np.ldexp(1.0, rng.integers(-12, 9, (N, CB))).repeat(BLOCK, axis=1)
    base = rng.standard_normal((N, C)).astype(F16)
    x = (base.astype(F32) + rng.standard_normal((N, C)) * mag).astype(F16)
    if nobase:
        x = (rng.standard_normal((N, C)) * mag).astype(F16)
    if case == "neighbours":
        # every other block of the flat view huge, the ones between tiny (nothing leaks from a block into its neighbours)
        huge = (rng.integers(0x7800, 0x7BFF + 1, (NB, BLOCK)).astype(np.uint16) | (rng.integers(0, 2, (NB, BLOCK)).astype(np.uint16) << 15)).view(F16)
        tiny = (rng.integers(0, 0x80, (NB, BLOCK)).astype(np.uint16) | (rng.integers(0, 2, (NB, BLOCK)).astype(np.uint16) << 15)).view(F16)
        blocks = list(np.where((np.arange(NB) % 2 == (rep % 2))[:, None], huge, tiny))
        pos = list(range(NB))
    else:
        blocks = _blocks(case, rng)
        take = blocks[rep * NB:(rep + 1) * NB] if len(blocks) > NB else blocks
        blocks, pos = take, BK._positions(len(take), NB)
    xf, bf = x.reshape(NB, BLOCK), base.reshape(NB, BLOCK)
    planted = np.zeros(NB, dtype=bool)
    for p, v in zip(pos, blocks):
        xf[p] = v
        bf[p] = 0
        planted[p] = True
    xb, bb = np.ascontiguousarray(x).view(np.uint16), np.ascontiguousarray(base).view(np.uint16)
    if bf16:
        sx, sb = _to_bf16_pair(x)
        pm = np.repeat(planted, BLOCK).reshape(N, C)
        xb = np.where(pm, sx, BK._f32_to_bf16(x.astype(F32)))
        bb = np.where(pm, sb, BK._f32_to_bf16(base.astype(F32)))
    return np.ascontiguousarray(xb), (None if nobase else np.ascontiguousarray(bb))


def planted(case, N, C, rep=0):
    """the blocks of the flat view that carry planted values"""
    NB = N * C // BLOCK
    if case == "neighbours":
        return list(range(NB))
    L = n_planted(case)
    take = min(NB, max(0, L - rep * NB)) if L > NB else L
    return BK._positions(take, NB)
