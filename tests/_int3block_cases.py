"""Deterministic inputs of the block-scaled 3-bit codec's suites (tests/test_int3block_contract.py on the CPU, tests/test_gpu_int3block.py on
the GPU).  The planting and the value cases are those of tests/_int2block_cases.py (and through it tests/_bblock_cases.py: the codecs share
lanes, block sum and scale): random, zero blocks of both signs and -0 deltas, subnormal means, +-65504 blocks, sums whose fp32 conversion
rounds, half-way means, a tiny block between huge ones, one nonzero element, all-equal blocks, an element at s, odd subnormal scales, scales
past 32752, bf16 states far beyond fp16.  Added here, for what the 3-bit codec has and the 2-bit one has not - three thresholds, four levels:
    at-thresholds        a block whose mean is s EXACTLY, with one element at each of t_0, t_1, t_2 = fp16(s * 0.75 / 1.5 / 2.625) and at the two
                         fp16 neighbours of each; s = (1 + m / 1024) 2^e with m small: for m != 0 a product s * T_k is no fp16 value and
                         rounds (m = 1: ties, to even)
    subnormal-thresholds the same around a subnormal s of a few units: s = 2^-24 gives t = 1, 2, 3 units (0.75 -> 1, 1.5 -> the tie, to 2) and
                         l_0 = fp16(0.375 units) = 0; thresholds that collide; all-equal blocks of 1 unit (|d| > t_0 fails: mag 0), 2, 3 units
    saturate-levels      s past 65504 / 3.375 with an element past t_2 (l_3 is 65504, not inf); s past 65504 / 2.625 (t_2 is 65504: mag 3 is out
                         of reach, the largest element is sent as mag 2); s past 65504 / 1.5 (mag 2 out of reach)
Shapes: SHAPES, what the GPU suite and the CPU contract test run, REPLACES tests/_int2block_cases.py's list by the smallest shapes at which
each index path of the kernels can go wrong (below, with what each one reaches); the shapes of that list which SHAPES drops - (3, 128),
(5, 192), (17, 384), (33, 1152) and BIG (129, 3072) - stay in the CPU contract test as INHERITED / BIG, where they cost no GPU time.  All
tensors are uint16 bit patterns, fp16 or bf16."""
import numpy as np

import _bblock_cases as BK
import _int2block_cases as I2

F16, F32 = np.float16, np.float32
BLOCKS = BK.BLOCKS
# (1, 64): one block, 8 live lanes; (1, 128): one block of 128; (3, 192), (5, 320): an odd number of blocks (the 16-bit scale tail), hi and lo
# words that end in the middle of a wave, E % 2048 != 0; (4, 2112): more than one workgroup of the stand-alone kernels and the 8192-element
# unit boundary of the layer's S group; (129, 128): two workgroups' boundaries and the 16384-element one of the D group
SHAPES = [(1, 64), (1, 128), (3, 192), (5, 320), (4, 2048 + 64), (129, 128)]
INHERITED = [s for s in I2.SHAPES if s not in SHAPES]           # CPU contract test only
BIG = I2.BIG                     # CPU contract test only: random values once per element type and block size
LAYER16 = BK.LAYER16             # once per element type: the 16-item layer (the FLUX shard)
blocks_of = BK.blocks_of
OWN = ["at-thresholds", "subnormal-thresholds", "saturate-levels"]
NAMES = I2.NAMES[:-1] + OWN + ["bf16"]
T = (0.75, 1.5, 2.625)


def _units(bits):
    """fp16 magnitude bits -> whole units of 2^-24 (Python integers)"""
    bits = int(bits)
    e, m = (bits >> 10) & 31, bits & 1023
    return (m | 1024) << (e - 1) if e else m


def _bits_of_units(u):
    """whole units of 2^-24 -> fp16 bits; the value must be an fp16 value"""
    v = F16(np.ldexp(float(u), -24))
    b = int(np.asarray(v).view(np.uint16))
    assert _units(b) == u, (u, b)
    return b


def _thr_bits(s_bits):
    """the three thresholds of a scale, as fp16 bits (float64 holds the products exactly; one rounding)"""
    s = float(np.asarray(s_bits, dtype=np.uint16).view(F16))
    return [int(np.asarray(F16(min(s * k, 65504.0))).view(np.uint16)) for k in T]


def _mean_block(B, s_bits, rng):
    """a block whose mean is s exactly: every threshold of s and its two fp16 neighbours, the rest spread evenly just below s, in steps of the
    ulp of the binade below s's (1 unit for a subnormal or lowest-binade s) so that every element is an fp16 value"""
    s_units = _units(s_bits)
    planted = []
    for t in _thr_bits(s_bits):
        planted += [t, t + 1] + ([t - 1] if t else [])
    mags = [_units(b) for b in planted]
    e = (s_bits >> 10) & 31
    g = 1 << max(e - 2, 0)                                      # the ulp of [s / 2, s)'s binade, in units
    n, rest = B - len(mags), B * s_units - sum(mags)
    assert rest >= 0 and rest % g == 0, (hex(s_bits), B)
    q, r = divmod(rest // g, n)
    mags += [(q + (i < r)) * g for i in range(n)]
    assert sum(mags) == B * s_units
    v = np.array([_bits_of_units(u) for u in mags], dtype=np.uint16)
    return (v | (rng.integers(0, 2, B).astype(np.uint16) << 15)).view(F16)


def _blocks(case, B, rng):
    out = []
    if case == "at-thresholds":
        for e in (15, 10, 25):                                  # s around 1, 2^-5 and 2^10
            for m in (0, 1, 2, 3, 5, 0x15):
                out.append(_mean_block(B, (e << 10) | m, rng))
    elif case == "subnormal-thresholds":
        for a in (1, 2, 3, 4, 5, 7, 0x155, 0x2AB, 0x3FF, 0x400, 0x401):
            out.append(_mean_block(B, a, rng))
        for a in (1, 2, 3):
            out.append(I2._signed(np.full(B, a), rng))
    elif case == "saturate-levels":
        for a in (0x74C0, 0x7700, 0x7A00):                      # 19456, 28672, 49152 everywhere and one 65504: l_3, t_2, t_1 saturate
            v = np.full(B, a)
            v[B // 2 + 1] = 0x7BFF
            out.append(I2._signed(v, rng))
        for k in (5, 6, 7, 11):                                 # k/16 of the block at 65504, the rest zero: s = 20470, 24564, 28658, 45034
            v = np.zeros(B, dtype=np.int64)
            v[rng.permutation(B)[:k * B // 16]] = 0x7BFF
            out.append(I2._signed(v, rng))
    else:
        raise AssertionError(case)
    return out


def cases_for(bf16):
    return NAMES if bf16 else [c for c in NAMES if c != "bf16"]


def n_planted(case, B):
    return len(_blocks(case, B, np.random.default_rng(0))) if case in OWN else I2.n_planted(case, B)


def reps(case, N, C, B):
    """repetitions a tensor of this shape needs to carry every planted block of the case"""
    return max(1, -(-n_planted(case, B) // (N * C // B)))


def build(case, N, C, B, bf16=False, rep=0, nobase=False, seed=0):
    """-> (x, base | None): uint16 bit patterns (N, C), fp16 or bf16"""
    if case not in OWN:
        return I2.build(case, N, C, B, bf16, rep, nobase, seed)
    x, base = BK.build("random", N, C, B, bf16, rep, nobase, seed + 101 + OWN.index(case))
    NB = N * C // B
    blocks = _blocks(case, B, np.random.default_rng([OWN.index(case), B, rep, seed]))
    take = blocks[rep * NB:(rep + 1) * NB] if len(blocks) > NB else blocks
    xf = x.reshape(NB, B)
    bf = None if base is None else base.reshape(NB, B)
    for p, v in zip(BK._positions(len(take), NB), take):
        if bf16:
            sx, sb = BK._split_bf16(v)
        else:
            sx, sb = np.ascontiguousarray(v).view(np.uint16), np.zeros(B, dtype=np.uint16)
        xf[p] = sx
        if bf is not None:
            bf[p] = sb
    return np.ascontiguousarray(xf.reshape(N, C)), (None if base is None else np.ascontiguousarray(bf.reshape(N, C)))
