"""Deterministic inputs of the block-scaled 1-bit codec's suites (tests/test_bblock_contract.py on the CPU, tests/test_gpu_bblock.py on the
GPU): the shapes at which the kernels can go wrong and the value cases of the contract (include/cfx.h, "BINARY_BLOCK").  A case plants whole
blocks of B deltas: on a planted block the state is +0, so that x - base is the planted value bit for bit (-0 - +0 = -0); everywhere else x
and base are random with block-wise magnitudes.  All tensors are uint16 bit patterns, fp16 or bf16.  For bf16 a planted fp16 delta v is split
into x = the top 8 significant bits of v and base = -(the rest), both bf16 values whose fp32 difference is v exactly (base None: x alone);
the case "bf16" is built in bf16 directly."""
import numpy as np

F16, F32 = np.float16, np.float32
BLOCKS = (32, 64, 128)

# (1, 64): 8 live lanes; (1, 128), (3, 128): one block of 128 a row; (5, 192): C no multiple of 128; (17, 384): E % 2048 != 0, a partly live
# last wave; (33, 1152): several workgroups, units of the layer's S (8192 elements) and D (16384) groups partly past the end
SHAPES = [(1, 64), (1, 128), (3, 128), (5, 192), (17, 384), (33, 1152)]
BIG = (129, 3072)                # once: 49 S workgroups and 25 D workgroups a tensor
LAYER16 = (544, 3072)            # the 16-item layer (the FLUX shard)


def blocks_of(N, C):
    """the block sizes a shape allows"""
    return [B for B in BLOCKS if C % max(B, 64) == 0]


def _h(bits):
    return np.asarray(bits, dtype=np.uint16).view(F16)


def _units(u):
    """a whole number of 2^-24 (below 1024: a subnormal) as fp16"""
    return _h(np.asarray(u, dtype=np.uint16))


def _blk(B, vals, fill=0.0):
    v = np.full(B, fill, dtype=F16)
    vals = np.asarray(vals, dtype=F16).reshape(-1)
    v[:vals.size] = vals
    return v


def _blocks(case, B, rng):
    """the planted blocks of a case: a list of B-vectors of fp16 deltas"""
    out = []
    if case == "zeros":
        out.append(np.zeros(B, dtype=F16))
        out.append(_h(np.full(B, 0x8000)))                                       # a block of -0
        out.append(_h(np.where(np.arange(B) % 2, 0x8000, 0)))
    elif case == "subnormals":
        # sums of B/2 - 1, B/2 (the tie between 0 and the smallest subnormal: even, 0), B/2 + 1, B, 3B/2 (tie: 2), 1 and 2B + 1 units,
        # then blocks of larger subnormals of both signs
        for total in (B // 2 - 1, B // 2, B // 2 + 1, B, 3 * B // 2, 1, 2 * B + 1, B * 1023):
            u = np.full(B, total // B, dtype=np.int64)
            u[:total - B * (total // B)] += 1
            rng.shuffle(u)
            assert u.sum() == total and u.max() < 1024
            out.append(_h(u.astype(np.uint16) | (rng.integers(0, 2, B).astype(np.uint16) << 15)))
        for top in (3, 0x200, 0x3FF):
            out.append(_h(rng.integers(0, top + 1, B).astype(np.uint16) | (rng.integers(0, 2, B).astype(np.uint16) << 15)))
    elif case == "max-65504":
        out.append(np.full(B, 65504, dtype=F16))
        out.append(np.full(B, -65504, dtype=F16))
        out.append((np.where(np.arange(B) % 3 == 0, -1, 1) * 65504.0).astype(F16))
    elif case == "sum-rounds":
        # sums past 2^24 .. 2^40 units whose fp32 conversion rounds: 2^T + 2^(T-11) lies half-way between two fp16 values once divided,
        # and k units of 2^(T-24) on top decide the fp32 rounding (k = 1: a tie, to even, back onto the fp16 tie; 3: past it; 0: exact)
        for T in (24, 25, 30, 37, 39):
            for k in (0, 1, 2, 3):
                for sign in (1.0, -1.0):
                    small = np.ldexp(1.0, T - 48)                                  # one unit of the fp32 rounding, as a value
                    vals = [sign * np.ldexp(1.0, T - 24), np.ldexp(1.0, T - 35)] + [-small] * k
                    assert all(float(F16(v)) == v for v in vals)
                    out.append(_blk(B, vals))
        # a full block of large values: the sum crosses 2^40 units (B x 32768 = 2^39 B), with a low element the fp32 sum cannot hold
        out.append(_blk(B, [_units([1])[0], 33.0], fill=32768.0))
        out.append(_blk(B, [-0.0078125, 32.0, -32800.0], fill=-32768.0))
    elif case == "half-way":
        # half the block at a, half at the next fp16 value: the mean is the tie between them (to the even one)
        for a in (0x3C00, 0x3C01, 0x0400, 0x03FF, 0x0001, 0x7BFE, 0x2BFF, 0x5555):
            v = np.where(np.arange(B) % 2, a + 1, a).astype(np.uint16) | (rng.integers(0, 2, B).astype(np.uint16) << 15)
            out.append(_h(v))
        # a quarter and three quarters of the way: not ties
        for a in (0x3C00, 0x3C01):
            out.append(_h(np.where(np.arange(B) % 4 == 0, a + 1, a).astype(np.uint16)))
            out.append(_h(np.where(np.arange(B) % 4 == 0, a, a + 1).astype(np.uint16)))
    elif case == "one-nonzero":
        # every lane of the block at one of its 8 slots, and every slot of the first and the last lane; signs alternate
        where = [8 * l + l % 8 for l in range(B // 8)] + list(range(8)) + list(range(B - 8, B))
        for j, pos in enumerate(where):
            v = np.zeros(B, dtype=F16)
            v[pos] = F16((-1.0 if j % 2 else 1.0) * np.ldexp(1.0 + (j % 7) / 8.0, (j % 25) - 12))
            out.append(v)
    else:
        assert case in ("random", "neighbours", "bf16"), case
    return out


NAMES = ["random", "zeros", "subnormals", "max-65504", "sum-rounds", "half-way", "neighbours", "one-nonzero", "bf16"]


def cases_for(bf16):
    return NAMES if bf16 else [c for c in NAMES if c != "bf16"]


def n_planted(case, B):
    return N_BF16_SPECIAL if case == "bf16" else len(_blocks(case, B, np.random.default_rng(0)))


def reps(case, N, C, B):
    """repetitions a tensor of this shape needs to carry every planted block of the case"""
    return max(1, -(-n_planted(case, B) // (N * C // B)))


def _positions(L, NB):
    """where the planted blocks go: spread over the tensor, the last one on the last block"""
    if L == 0:
        return []
    step = max(1, NB // L)
    pos = [(k * step) % NB for k in range(L)]
    pos[-1] = NB - 1
    return pos


def _f32_to_bf16(f32):
    u = np.ascontiguousarray(f32, dtype=F32).view(np.uint32)
    return ((u + (0x7FFF + ((u >> 16) & 1))) >> 16).astype(np.uint16)


def _split_bf16(v16):
    """fp16 deltas -> bf16 bits (x, base) with fp32(x) - fp32(base) == v exactly and the sign of a zero kept"""
    u = np.ascontiguousarray(v16, dtype=F16).astype(F32).view(np.uint32)
    hi = (u & np.uint32(0xFFFF0000)).view(F32)
    lo = v16.astype(F32) - hi                                                    # exact: the low 3 bits of the significand
    xb = (hi.view(np.uint32) >> 16).astype(np.uint16)
    nlo = (-lo).astype(F32)
    bb = np.where(lo == 0, np.uint16(0), (nlo.view(np.uint32) >> 16).astype(np.uint16))      # (x - (+0) keeps -0)
    assert np.array_equal((nlo.view(np.uint32) & 0xFFFF), np.zeros_like(u))
    return xb, bb


N_BF16_SPECIAL = 4


def _bf16_direct(N, C, B, rng, rep):
    """x and base far beyond fp16 with a small difference; |d| up to 65504 exactly; round-to-even ties of the bf16 state"""
    NB = N * C // B
    e = rng.choice(np.array([17, 18, 19, 20, 20, 19, 18, 40, 100]), (NB, 1))     # base ~ 2^17 .. 2^100: no fp16 value
    m = rng.integers(128, 256, (NB, B))
    base = np.ldexp(m.astype(np.float64), e - 7) * np.where(rng.integers(0, 2, (NB, B)), -1.0, 1.0)
    # x = base + j ulps of bf16 at base's binade, |j| <= 7: exact in fp32; where 7 ulps are past 65504 the delta would leave fp16: j = 0 there
    j = rng.integers(-7, 8, (NB, B))
    ulp = np.ldexp(1.0, e - 7)
    j = np.where(ulp * 7 > 65504, 0, j)
    xf = base + j * ulp
    xf = np.where(np.abs(xf) >= np.ldexp(1.0, e + 1), base, xf)                  # (stay below the next binade: x is a bf16 value)
    x, b = xf.astype(F32), base.astype(F32)
    special = []
    # |d| = 65504 = 65280 - (-224), and its negative
    sx, sb = np.full(B, 65280.0), np.full(B, -224.0)
    sx[1::2], sb[1::2] = -65280.0, 224.0
    special.append((sx, sb))
    # ties of the state: half the block moves by 2^(p-7), the other half not at all - the mean is 2^(p-8), half an ulp of bf16 at 2^p, and
    # base + recv lies half-way between two bf16 values for every element that did not move (last bits of base 00, 01, 10, 11)
    for p in (0, 5, -9):
        bb = np.ldexp((128 + (np.arange(B) % 4)).astype(np.float64), p - 7)
        move = np.where(np.arange(B) % 8 < 4, np.where(np.arange(B) % 2, -1.0, 1.0) * np.ldexp(1.0, p - 7), 0.0)
        special.append((bb + move, bb))
    assert len(special) == N_BF16_SPECIAL
    take = special[rep * NB:(rep + 1) * NB] if len(special) > NB else special
    for pos, (sx, sb) in zip(_positions(len(take), NB), take):
        x[pos, :], b[pos, :] = sx.astype(F32), sb.astype(F32)
    xb, bb = _f32_to_bf16(x), _f32_to_bf16(b)
    assert np.array_equal((xb.astype(np.uint32) << 16).view(F32), x) and np.array_equal((bb.astype(np.uint32) << 16).view(F32), b)
    return xb.reshape(N, C), bb.reshape(N, C)


def build(case, N, C, B, bf16=False, rep=0, nobase=False, seed=0):
    """-> (x, base | None): uint16 bit patterns (N, C), fp16 or bf16"""
    assert C % max(B, 64) == 0 and (bf16 or case != "bf16")
    rng = np.random.default_rng([NAMES.index(case), N, C, B, rep, seed, int(bf16)])
    NB, CB = N * C // B, C // B
    if case == "bf16":
        x, base = _bf16_direct(N, C, B, rng, rep)
        if nobase:                                               # the differences themselves, cut to bf16: small values with no state
            d = (x.astype(np.uint32) << 16).view(F32) - (base.astype(np.uint32) << 16).view(F32)
            return np.ascontiguousarray((d.view(np.uint32) >> 16).astype(np.uint16)), None
        return x, base
    mag = np.ldexp(1.0, rng.integers(-12, 9, (N, CB))).repeat(B, axis=1)
    base = rng.standard_normal((N, C)).astype(F16)
    x = (base.astype(F32) + rng.standard_normal((N, C)) * mag).astype(F16)
    if nobase:
        x = (rng.standard_normal((N, C)) * mag).astype(F16)
    if case == "neighbours":
        # every other block of the flat view huge, the ones between tiny: a block between two of the other kind, and the last block of a
        # row against the first of the next (a row of an odd number of blocks, or of one block, alternates across the row boundary too)
        huge = (rng.integers(0x7800, 0x7BFF + 1, (NB, B)).astype(np.uint16) | (rng.integers(0, 2, (NB, B)).astype(np.uint16) << 15)).view(F16)
        tiny = (rng.integers(0, 0x40, (NB, B)).astype(np.uint16) | (rng.integers(0, 2, (NB, B)).astype(np.uint16) << 15)).view(F16)
        blocks = list(np.where((np.arange(NB) % 2 == (rep % 2))[:, None], huge, tiny))
        pos = list(range(NB))
    else:
        blocks = _blocks(case, B, rng)
        take = blocks[rep * NB:(rep + 1) * NB] if len(blocks) > NB else blocks
        blocks, pos = take, _positions(len(take), NB)
    xf, bf = x.reshape(NB, B), base.reshape(NB, B)
    planted = np.zeros(NB, dtype=bool)
    for p, v in zip(pos, blocks):
        xf[p] = v
        bf[p] = 0
        planted[p] = True
    xb, bb = np.ascontiguousarray(x).view(np.uint16), np.ascontiguousarray(base).view(np.uint16)
    if bf16:
        sx, sb = _split_bf16(x)
        pm = np.repeat(planted, B).reshape(N, C)
        xb = np.where(pm, sx, _f32_to_bf16(x.astype(F32)))
        bb = np.where(pm, sb, _f32_to_bf16(base.astype(F32)))
    return np.ascontiguousarray(xb), (None if nobase else np.ascontiguousarray(bb))
