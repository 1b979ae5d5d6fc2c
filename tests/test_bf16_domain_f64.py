"""The bf16 contract (tests/bf16_contract.py: the pinned oracle between two conversions) against the bf16 DEFINITION checked
independently (tests/_bf16_f64_check.py: float64 bounds on d, torch's bf16 rounding of the fp32 sum) over every legal shape of
tests/_domain_cases.py and every value case of tests/_bf16_cases.py - what tests/test_gpu_bf16_domain.py then holds the kernels to.
Also: the check rejects planted errors, and the value domain contains every kind of case it claims.  CPU only."""
import numpy as np
import pytest

import _bf16_cases as V
import _bf16_f64_check as BF
import _domain_cases as D
import bf16_contract as BC

NAMES = ("binary", "int2")
F16 = np.float16


def shape_inputs(seed, N, C):
    rng = np.random.default_rng(seed)
    base = V.bf16_bits(0.5 * rng.standard_normal((N, C)))
    x = V.bf16_bits(V.bf16_f32(base) + 0.2 * rng.standard_normal((N, C)).astype(np.float32))
    return x, base


def _finite(u16):
    return ((np.asarray(u16).view(np.uint16) & 0x7F80) != 0x7F80).all()


SHAPE_CASES = [pytest.param(n, N, C, id=f"{n}-{N}x{C}") for n in NAMES for N, C in D.shapes_for(n) + [V.LAYER] if N * C <= 4 << 20]
BIG_SHAPES = [pytest.param(n, N, C, id=f"{n}-{N}x{C}") for n in NAMES for N, C in D.shapes_for(n) if N * C > 4 << 20]


@pytest.mark.parametrize("name,N,C", SHAPE_CASES + BIG_SHAPES)
def test_contract_meets_the_definition_on_every_legal_shape(name, N, C):
    x, base = shape_inputs(N * 131 + C, N, C)
    pkt, nb = BC.compress(name, x, base)
    BF.check(name, x, base, pkt, nb)
    assert np.array_equal(BC.decompress(name, pkt, base, N, C), nb)
    if N * C <= 1 << 20:
        pkt0, nb0 = BC.compress(name, x, None)
        BF.check(name, x, None, pkt0, nb0)


VALUE_CASES = [pytest.param(n, c, N, C, id=f"{n}-{c}-{N}x{C}") for n in NAMES for c, N, C in V.all_cases()]


@pytest.mark.parametrize("name,case,N,C", VALUE_CASES)
def test_contract_meets_the_definition_on_every_value_case(name, case, N, C):
    x, base = V.build(case, N, C)
    pkt, nb = BC.compress(name, x, base)
    assert _finite(nb) and np.isfinite(np.asarray(pkt).view(F16)[-(N + C):]).all(), "the case leaves the finite domain"
    BF.check(name, x, base, pkt, nb)
    rec = BC.decompress(name, pkt, base, N, C)
    assert np.array_equal(rec, nb)
    BF.check_state(name, base, pkt, rec)


@pytest.mark.parametrize("N,C", V.TIE_SHAPES)
@pytest.mark.parametrize("name", NAMES)
def test_contract_meets_the_definition_on_the_tie_packets(name, N, C):
    base, pkt = V.tie_packet(name, N, C)
    BF.check_state(name, base, pkt, BC.decompress(name, pkt, base, N, C))
    BF.check_state(name, None, pkt, BC.decompress(name, pkt, None, N, C))
    if name == "int2":
        x, b, tok, chan = V.tie_quantize(N, C)
        p, nb = BC.int2_quantize(x, b, tok, chan)
        BF.check_state("int2", b, p, nb)
        d = BF.delta16(x, b)
        idx = ((np.asarray(p).view(np.uint8)[:N * C // 4].reshape(N, C // 4)[:, :, None] >> (2 * np.arange(4, dtype=np.uint8))) & 3).reshape(N, C)
        thr = (chan.reshape(1, -1) * tok.reshape(-1, 1)).astype(F16)
        assert np.array_equal(idx >> 1, d >= 0) and np.array_equal((idx & 1).astype(bool), np.abs(d) > thr)


# ---- the check rejects planted errors ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_check_rejects_planted_errors(name):
    N, C = 129, 144
    x, base = shape_inputs(5, N, C)
    pkt, nb = BC.compress(name, x, base)
    BF.check(name, x, base, pkt, nb)
    nbytes = {"binary": N * C // 8, "int2": N * C // 4}[name]
    # one flipped sign bit
    bad = pkt.copy()
    bad.view(np.uint8)[nbytes // 2] ^= 0x80 if name == "binary" else 0x02
    with pytest.raises(AssertionError, match="sign bits"):
        BF.check(name, x, base, bad, None)
    # one state element one bf16 ulp off
    bad = nb.copy()
    bad[77, 5] += 1
    with pytest.raises(AssertionError, match="1/18576 state elements"):
        BF.check(name, x, base, pkt, bad)
    # a state rounded toward zero instead of to nearest even
    recv = BF.decode(name, pkt, N, C)
    s32 = V.bf16_f32(base) + recv.astype(np.float32)
    trunc = (s32.view(np.uint32) >> 16).astype(np.uint16)
    assert 0.2 < (trunc != nb).mean() < 0.8
    with pytest.raises(AssertionError, match="state elements"):
        BF.check(name, x, base, pkt, trunc)
    # a V / chan scale 2 ulp off
    bad = pkt.copy()
    bad[nbytes // 2 + N + 40] += 2
    with pytest.raises(AssertionError, match="column means"):
        BF.check(name, x, base, bad, None)
    # the two-step state: base = 2^-30, recv = 1 + 2^-8 (an fp16 value, and a bf16 tie).  The fp32 sum rounds to recv, the tie goes to even:
    # 1.0.  One rounding of the exact sum would see the base and go up to 1 + 2^-7: not the definition
    b1 = V._exact(np.full((2, 8), 2.0 ** -30, np.float32))
    col = np.full(8, (1.0 + 2.0 ** -8) * (2.0 if name == "int2" else 1.0), F16)
    codes = np.full(2 if name == "binary" else 4, 0xFF if name == "binary" else 0xAA, np.uint8)          # every sign bit 1, magnitude bits 0
    p1 = np.concatenate([codes, np.ones(2, F16).view(np.uint8), col.view(np.uint8)]).view(np.uint16)
    got = BC.decompress(name, p1, b1, 2, 8)
    assert (got == 0x3F80).all()
    BF.check_state(name, b1, p1, got)
    with pytest.raises(AssertionError, match="state elements"):
        BF.check_state(name, b1, p1, np.full((2, 8), 0x3F81, np.uint16))


def test_the_double_rounding_corner_is_refused_not_decided():
    """x = 2.5 * 2^-24 with base = -2^-60: the exact difference rounds to 3 units of 2^-24, the contract's fp32 difference is x itself, a tie,
    and rounds to 2.  The check's d is defined where the two agree; the value domain stays there (every value case passes delta16)."""
    x = V._exact(np.array([[2.5 * 2.0 ** -24] * 8], np.float32))
    b = V._exact(np.array([[-(2.0 ** -60)] * 8], np.float32))
    assert BC.delta(x, b).view(np.uint16)[0, 0] == 2
    with pytest.raises(AssertionError, match="single rounding"):
        BF.delta16(x, b)


# ---- the value domain has every kind of case ---------------------------------------------------------------------------------------
def _ties(base, recv16):
    """(ties with an even lower neighbour, with an odd one) among fp32(base) + fp32(recv): the fp32 sum exact and its low 16 bits 0x8000"""
    b64, r64 = BF.widen64(base), recv16.astype(np.float64)
    s32 = V.bf16_f32(base) + recv16.astype(np.float32)
    u = s32.view(np.uint32)
    tie = (s32.astype(np.float64) == b64 + r64) & ((u & 0xFFFF) == 0x8000)
    return int((tie & ((u >> 16) & 1 == 0)).sum()), int((tie & ((u >> 16) & 1 == 1)).sum())


def test_value_domain_has_every_case_kind():
    """every generator at two or three shapes, one of them taking the one-launch layer form and one not; ties of both parities (from the
    hand-built packets and from cfx_int2_quantize's planted scales); an fp16-subnormal d; a -0 d and a -0 state; tile sums past 2^32 and
    2^40 units of 2^-24 (a row's 512-channel block, and a column over a 32-row tile); |d| above 65000; |x| above 2^21"""
    for name, shapes, why in V.CASES:
        assert 2 <= len(shapes) <= 3 and why, name
        assert any(C % 128 == 0 and N % 32 == 0 for N, C in shapes), name
        assert any(C % 128 for N, C in shapes) or name.startswith("drift"), name
        for N, C in shapes:
            assert D.legal("binary", N, C) and D.legal("int2", N, C)
    for name in NAMES:
        even = odd = 0
        for N, C in V.TIE_SHAPES:
            base, pkt = V.tie_packet(name, N, C)
            e, o = _ties(base, BF.decode(name, pkt, N, C))
            assert e > N * C // 16 and o > N * C // 16, (name, N, C, e, o)
            st = BC.decompress(name, pkt, None, N, C)
            assert (st[:, 0:8] == 0x8000).any() and (st[:, 0:8] == 0).any(), "no signed zero state from a zero scale"
        assert any(C % 128 == 0 for _, C in V.TIE_SHAPES) and any(C % 128 for _, C in V.TIE_SHAPES)
    x, b, tok, chan = V.tie_quantize(*V.LAYER)
    p, _ = BC.int2_quantize(x, b, tok, chan)
    e, o = _ties(b, BF.decode("int2", p, *V.LAYER))
    assert e > 1000 and o > 1000, (e, o)
    seen = set()
    for case, N, C in V.all_cases():
        x, base = V.build(case, N, C)
        d = BF.delta16(x, base)
        ad = np.abs(d.astype(np.float64))
        if ((ad > 0) & (ad < 2.0 ** -14)).any():
            seen.add("fp16-subnormal d")
        if (d.view(np.uint16) == 0x8000).any():
            seen.add("-0 d")
        if (ad > 65000).any():
            seen.add("|d| near 65504")
        if (np.abs(V.bf16_f32(x)) > 2.0 ** 21).any():
            seen.add("|x| beyond fp16")
        if ((x & 0x7F80) == 0).any() and ((x & 0x7FFF) != 0).any() and (((x & 0x7F80) == 0) & ((x & 0x7F) != 0)).any():
            seen.add("bf16 subnormal")
        units = ad * 2.0 ** 24
        pad = (-C) % 512
        rowp = np.pad(units, ((0, 0), (0, pad))).reshape(N, -1, 512).sum(axis=2).max()
        colp = np.pad(units, ((0, (-N) % 32), (0, 0))).reshape(-1, 32, C).sum(axis=1).max()
        for kind, v in (("row", rowp), ("column", colp)):
            if v > 2.0 ** 32:
                seen.add(f"{kind} partial past 2^32")
            if v > 2.0 ** 40:
                seen.add(f"{kind} partial past 2^40")
        if base is None:
            _, nb = BC.compress("binary", x, None)
            if (nb == 0x8000).any():
                seen.add("-0 state without a base")
        if (ad.sum(axis=1) == 0).any() and (ad.sum(axis=0) == 0).any():
            seen.add("zero rows and columns")
        assert ad.sum() > 0
    want = {"fp16-subnormal d", "-0 d", "|d| near 65504", "|x| beyond fp16", "bf16 subnormal", "row partial past 2^32", "row partial past 2^40",
            "column partial past 2^32", "column partial past 2^40", "-0 state without a base", "zero rows and columns"}
    assert seen == want, want - seen
