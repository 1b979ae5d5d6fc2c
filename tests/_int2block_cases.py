"""Deterministic inputs of the block-scaled 2-bit codec's suites (tests/test_int2block_contract.py on the CPU, tests/test_gpu_int2block.py on
the GPU).  The shapes and the planting are those of tests/_bblock_cases.py - the two codecs share lanes, block sum and scale - and so are its
value cases (random, zero blocks of both signs and -0 deltas, subnormal means, +-65504 blocks where s = 65504 and no magnitude bit is set,
sums whose fp32 conversion rounds, half-way means, a tiny block between huge ones, one nonzero element, bf16 states far beyond fp16 with
round-to-even ties).  Added here, for what the 2-bit codec has and the 1-bit one has not - the strict threshold and the two levels:
    all-equal      every |d| of the block is s itself: no magnitude bit (the compare is strict)
    at-threshold   one element exactly at s, its two fp16 neighbours beside it (the mean stays s exactly): codes 0, 1, 0
    odd-scale      s subnormal or in the lowest binade with an odd significand: 0.5 s is a tie, to even; s = 2^-24: small = 0
    saturate       s in (32752, 65504] with an element above it: 2 s is past fp16, large = 65504; s = 32752: 2 s = 65504 exactly
All tensors are uint16 bit patterns, fp16 or bf16."""
import numpy as np

import _bblock_cases as BK

F16, F32 = np.float16, np.float32
BLOCKS, SHAPES, BIG, LAYER16 = BK.BLOCKS, BK.SHAPES, BK.BIG, BK.LAYER16
blocks_of = BK.blocks_of
OWN = ["all-equal", "at-threshold", "odd-scale", "saturate"]
NAMES = BK.NAMES[:-1] + OWN + ["bf16"]


def _signed(mag_bits, rng):
    mag_bits = np.asarray(mag_bits, dtype=np.uint16)
    return (mag_bits | (rng.integers(0, 2, mag_bits.size).astype(np.uint16) << 15)).view(F16)


def _around(B, a, up, down, rng):
    """a block of magnitude bits a whose mean stays a exactly: `up` elements k steps above, as many steps taken off `down` elements"""
    v = np.full(B, a, dtype=np.int64)
    i = 1                                                       # (element 0 stays at a: the element AT the threshold)
    for k in up:
        v[i] += k
        i += 1
    for k in down:
        v[i] -= k
        i += 1
    return _signed(v, rng)


def _blocks(case, B, rng):
    out = []
    if case == "all-equal":
        for a in (0x3C00, 0x0001, 0x03FF, 0x0400, 0x3555, 0x7BFF, 0x77FF, 0x7800):
            out.append(_signed(np.full(B, a), rng))
    elif case == "at-threshold":
        # a, a + 1 ulp, a - 1 ulp, the rest a: inside one binade (or across 0x0400, where subnormals and the lowest binade share their ulp) the
        # magnitudes are an arithmetic progression, the sum B a and the mean a.  0x7BFE: the upper neighbour is 65504 and 2 s saturates
        for a in (0x3C10, 0x0400, 0x0005, 0x7BFE, 0x5801, 0x2BFE, 0x0002):
            out.append(_around(B, a, [1], [1], rng))
            if 4 <= a < 0x7BFE:
                out.append(_around(B, a, [1, 2], [3], rng))
    elif case == "odd-scale":
        # s = a units of 2^-24 (a below 1024) or a in the lowest binade: 0.5 s has half a unit to round - 1 -> 0, 3 -> 2, 5 -> 2, 0x3FF -> 0x200,
        # 0x401 -> 0x200, 0x7FF -> 0x400; one element above s sends `large` beside them
        for a in (1, 3, 5, 7, 0x3FF, 0x3FD, 0x401, 0x403, 0x7FF, 2, 0x400):
            out.append(_signed(np.full(B, a), rng))
            out.append(_around(B, a, [1], [1], rng))
    elif case == "saturate":
        v = np.full(B, 0x7A00)                                  # 49152 everywhere, one 65504: s a little above 49152
        v[B // 2] = 0x7BFF
        out.append(_signed(v, rng))
        out.append(_around(B, 0x7800, [1], [1, 1], rng))        # s = 32768 (32800 and twice 32752 beside it: ulps 32 and 16): 2 s = 65536
        out.append(_around(B, 0x77FF, [1], [1], rng))           # s = 32752: 2 s = 65504 exactly, not saturated
        out.append(_around(B, 0x7801, [1], [1], rng))           # s = 32800: saturated
        v = np.full(B, 0x7BFF)                                  # 65504 everywhere but one zero: s just below 65504, every other element above it
        v[3] = 0
        out.append(_signed(v, rng))
    else:
        raise AssertionError(case)
    return out


def cases_for(bf16):
    return NAMES if bf16 else [c for c in NAMES if c != "bf16"]


def n_planted(case, B):
    return len(_blocks(case, B, np.random.default_rng(0))) if case in OWN else BK.n_planted(case, B)


def reps(case, N, C, B):
    """repetitions a tensor of this shape needs to carry every planted block of the case"""
    return max(1, -(-n_planted(case, B) // (N * C // B)))


def build(case, N, C, B, bf16=False, rep=0, nobase=False, seed=0):
    """-> (x, base | None): uint16 bit patterns (N, C), fp16 or bf16"""
    if case not in OWN:
        return BK.build(case, N, C, B, bf16, rep, nobase, seed)
    x, base = BK.build("random", N, C, B, bf16, rep, nobase, seed + 1 + OWN.index(case))
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
