"""Deterministic inputs of the MXFP4 suites (tests/test_mxfp4_contract.py on the CPU, tests/test_gpu_mxfp4.py on the GPU): the shapes at which
the kernels can go wrong and the value cases of the contract (include/cfx.h, "MXFP4").  A case plants whole blocks of 32 deltas: on a planted
block the state is +0, so that fp16(x - base) is the planted value bit for bit (-0 - +0 = -0); everywhere else x and base are random with
block-wise magnitudes.  A tensor with fewer blocks than a case has planted blocks takes them over `reps(case, N, C)` repetitions."""
import numpy as np

F16 = np.float16
BLOCK = 32

# (1, 64): 8 live lanes; (5, 320): the last wave partial; (17, 576): just past one S workgroup of the layer launch (8192 elements);
# (8, 1024), (32, 128): the shapes of the existing layer-form tests; (64, 3072): 24 S workgroups, 12 D workgroups a tensor
SHAPES = [(1, 64), (3, 64), (2, 192), (5, 320), (33, 128), (17, 576), (8, 1024), (32, 128), (64, 3072)]
LAYER16 = (544, 3072)            # the 16-item layer (the FLUX shard)
MIDPOINTS = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)


def _h(bits):
    return np.asarray(bits, dtype=np.uint16).view(F16)


def _fill(vals, rng, small):
    """a block of 32: `vals` first, the rest random and at most `small` in magnitude (fp16 bits compare as magnitudes)"""
    v = np.zeros(BLOCK, dtype=F16)
    vals = np.asarray(vals, dtype=F16).reshape(-1)
    assert vals.size <= BLOCK
    v[:vals.size] = vals
    if small is not None and vals.size < BLOCK:
        sb = int(np.asarray(small, dtype=F16).view(np.uint16)) & 0x7FFF
        r = rng.integers(0, sb + 1, BLOCK - vals.size).astype(np.uint16) | (rng.integers(0, 2, BLOCK - vals.size).astype(np.uint16) << 15)
        v[vals.size:] = _h(r)
    return v


def _blocks(case, rng):
    """the planted blocks of a case: a list of 32-vectors"""
    out = []
    if case == "zeros":
        out.append(np.zeros(BLOCK, dtype=F16))
        out.append(_h(np.full(BLOCK, 0x8000)))                                   # a block of -0
        out.append(_h(np.where(np.arange(BLOCK) % 2, 0x8000, 0)))
    elif case == "negative-to-zero":
        for k in (-12, 0, 9):
            m = np.ldexp(1.0, k)
            out.append(_fill([6 * m, -0.25 * m, -0.2 * m, -0.01 * m, 0.25 * m, -0.0, -0.2500001 * m, -0.26 * m, 0.2 * m], rng, None))
    elif case == "subnormal-max":
        for a in (1, 7, 8, 0x3FF, 2, 9, 15, 16, 0x200, 0x400, 0x401):
            for sign in (0, 0x8000):
                v = rng.integers(0, a + 1, BLOCK).astype(np.uint16)
                v[rng.integers(0, BLOCK)] = a
                out.append(_h(v | np.uint16(sign) * (np.arange(BLOCK) % 3 == 0).astype(np.uint16)))
        # under the clamp (X = -23) y is a multiple of 0.5: the ties 2.5, 3.5 and 5 are the bits 5, 7 and 10
        out.append(_h(np.arange(BLOCK) % 16))
        out.append(_h((np.arange(BLOCK) % 16) | 0x8000))
    elif case == "power-of-two-max":
        for k in range(-24, 16):
            m = np.ldexp(1.0, k)
            out.append(_fill([m, -m, m / 2, m / 4, m / 8, m / 16, m / 32, 3 * m / 4, -3 * m / 8, 5 * m / 8], rng, m))
    elif case == "saturation":
        for k in range(-16, 14):
            m = np.ldexp(1.0, k)
            top = _h([((k + 2 + 15) << 10) | 0x3FF])[0] if k + 2 + 15 >= 1 else F16(7.99 * m)      # the largest value below 8 * 2^k
            for big in (6 * m, 7 * m, top, 6.5 * m, 7.5 * m):
                out.append(_fill([big, -big, 5 * m, 5.5 * m, 6 * m, -6 * m], rng, 4 * m))
    elif case == "midpoints":
        for X in (-22, -20, -14, -8, 0, 5, 12, 13):
            m = np.ldexp(1.0, X)
            for sign in (1.0, -1.0):
                mids = np.array([sign * p * m for p in MIDPOINTS], dtype=F16)
                assert np.array_equal(mids.astype(np.float64), [sign * p * m for p in MIDPOINTS])
                mb = mids.view(np.uint16)
                vals = np.concatenate([np.array([6 * m], dtype=F16), mids, _h(mb - 1), _h(mb + 1)])
                out.append(_fill(vals, rng, None))
    elif case == "max-65504":
        out.append(_fill([65504, -65504, 49152, 40960, 45056, 45060, 8192 * 0.25, -8192 * 5], rng, 60000))
        out.append(_fill([-65504, 1, 2, 3], rng, 2048))
    elif case == "max-position":
        for pos in range(BLOCK):                                                 # each of the 4 lanes, each of a lane's 8 slots
            v = _fill([], rng, 1.0)
            v[pos] = F16(-3.0 if pos % 2 else 3.0) * F16(16.0)
            out.append(v)
    elif case == "binades-apart":
        for j in range(8):
            out.append(_fill([np.ldexp(1.5, 10 if j % 2 else -10)], rng, np.ldexp(1.0, 10 if j % 2 else -10)))
    elif case == "overflow":
        out.append(_fill([1.0, -2.0, 0.5], rng, 1.0))                            # (build() makes its first delta overflow)
    elif case == "nonfinite":
        v = _fill([1.0, np.nan, np.inf, -3.0], rng, 8.0)
        out += [v, _fill([-np.inf, 2.0], rng, 2.0), _fill([np.nan], rng, 2.0)]
    else:
        assert case in ("random", "edges"), case
    return out


NAMES = ["random", "zeros", "negative-to-zero", "subnormal-max", "power-of-two-max", "saturation", "midpoints", "max-65504", "max-position",
         "binades-apart", "edges", "overflow", "nonfinite"]
FINITE = [c for c in NAMES if c not in ("overflow", "nonfinite")]


def n_planted(case):
    return len(_blocks(case, np.random.default_rng(0)))


def reps(case, N, C):
    """repetitions a tensor of this shape needs to carry every planted block of the case"""
    nb = N * C // BLOCK
    return max(1, -(-n_planted(case) // nb))


def _positions(L, NB, CB):
    """where the planted blocks go: spread over the tensor, the first at the first columns of a row and the last at the last columns"""
    if L == 0:
        return []
    step = max(1, NB // L)
    pos = [(k * step) % NB for k in range(L)]
    pos[-1] = NB - 1
    return pos


def build(case, N, C, rep=0, nobase=False, seed=0):
    """-> (x, base | None) fp16 (N, C).  planted(case, N, C, rep) says which blocks carry planted values."""
    rng = np.random.default_rng([NAMES.index(case), N, C, rep, seed])
    NB, CB = N * C // BLOCK, C // BLOCK
    mag = np.ldexp(1.0, rng.integers(-12, 9, (N, CB))).repeat(BLOCK, axis=1)
    with np.errstate(over="ignore"):
        base = rng.standard_normal((N, C)).astype(F16)
        x = (base.astype(np.float32) + rng.standard_normal((N, C)) * mag).astype(F16)
    if nobase:
        x = (rng.standard_normal((N, C)) * mag).astype(F16)
    blocks = _blocks(case, rng)
    if case == "edges":                                     # special values on the first and the last block of every row
        src = _blocks("midpoints", rng) + _blocks("saturation", rng)
        blocks = [src[(rep * 2 * N + i) % len(src)] for i in range(2 * N)]
        pos = [n * CB + j for n in range(N) for j in (0, CB - 1)]
    else:
        take = blocks[rep * NB:(rep + 1) * NB] if len(blocks) > NB else blocks
        blocks, pos = take, _positions(len(take), NB, CB)
    xf, bf = x.reshape(NB, BLOCK), base.reshape(NB, BLOCK)
    for p, v in zip(pos, blocks):
        xf[p] = v
        bf[p] = 0
    if case == "overflow" and blocks:
        p = pos[0]
        if nobase:
            xf[p, 0] = np.inf
        else:
            xf[p, 0], bf[p, 0] = F16(65504), F16(-65504)   # x - base overflows: an inf delta
    return np.ascontiguousarray(x), (None if nobase else np.ascontiguousarray(base))


def planted(case, N, C, rep=0):
    NB, CB = N * C // BLOCK, C // BLOCK
    if case == "edges":
        return [n * CB + j for n in range(N) for j in (0, CB - 1)]
    L = n_planted(case)
    take = min(NB, max(0, L - rep * NB)) if L > NB else L
    return _positions(take, NB, CB)
