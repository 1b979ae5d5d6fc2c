"""The contract of the INT2_MINMAX wire codec (include/cfx.h, CFX_CODEC_INT2_MINMAX = 6) in numpy, on top of oracle.ref_np - the statement
the kernels are held to.  INT4's arithmetic with 4 levels, one fp16 rounding per reference operation (compress_quantize.py:386-426):

    d = x - base ; scale, min = _minmax_scale(d, 3 + 1e-6) ; q = clamp(rint(fp16(fp16(d - min) / scale)), 0, 3), a NaN quotient -> 0
    recv = fp16(fp16(q * scale) + min) ; wire [ codes (N/4, C) bytes, q[4k+h][c] at bits 2h | scale C | min C ]

Where R.sim_int2_minmax(d) is finite, recv equals it bit for bit; on a channel whose deltas are all equal (scale 0, NaN quotient) the wire
codec stores code 0 and reconstructs `min`.  Plain helper module (no tests here: tests/test_int2mm_contract.py holds it to the pinned
function and to the float64 definition)."""
import numpy as np

from oracle import ref_np as R

F16, F32, F64 = np.float16, np.float32, np.float64
NAME, CID, LEVELS = "int2mm", 6, 3


def packet_halves(N, C):
    return N * C // 8 + 2 * C


def codes(d16, scale16, min16):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = ((d16 - min16).astype(F16) / scale16).astype(F16)
        q = np.clip(np.rint(t).astype(F16), F16(0), F16(LEVELS))
    return R._nan_to_zero_int(q, np.uint8)


def pack(q):
    N, C = q.shape
    assert N % 4 == 0
    q = q.reshape(N // 4, 4, C)
    return ((q[:, 0] & 3) | ((q[:, 1] & 3) << 2) | ((q[:, 2] & 3) << 4) | ((q[:, 3] & 3) << 6)).astype(np.uint8)


def unpack(packed):
    N4, C = packed.shape
    out = np.empty((N4 * 4, C), dtype=np.uint8)
    for h in range(4):
        out[h::4] = (packed >> (2 * h)) & 3
    return out


def recv_of(q, scale16, min16):
    with np.errstate(invalid="ignore", over="ignore"):
        return ((q.astype(F16) * scale16).astype(F16) + min16).astype(F16)


def compress(x, base):
    """-> (packet words uint16, recv fp16 (N, C)); recv = decompress(packet) exactly"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = R._delta(x, base)
    N, C = d.shape
    assert N % 4 == 0 and C % 8 == 0
    scale, mn = R._minmax_scale(d, LEVELS + 1e-6)
    q = codes(d, scale, mn)
    pkt = np.concatenate([R._as_half_words(pack(q)), R.bits(scale).reshape(-1), R.bits(mn).reshape(-1)])
    assert pkt.size == packet_halves(N, C)
    return pkt, recv_of(q, scale, mn)


def decompress(packet, N, C):
    """packet words -> recv (N, C) fp16 (no base add)"""
    w = np.asarray(packet).view(np.uint16).reshape(-1)
    assert w.size == packet_halves(N, C), (w.size, packet_halves(N, C))
    qn = N * C // 8
    q = unpack(w[:qn].view(np.uint8).reshape(N // 4, C))
    return recv_of(q, w[qn:qn + C].view(F16).reshape(1, C), w[qn + C:].view(F16).reshape(1, C))


def residual_compress(x, base, ef=True):
    """(packet, new_base) as R.residual_compress"""
    pkt, recv = compress(x, base)
    return pkt, (R._add_base(base, recv) if ef else R.as_f16(x).copy())


def residual_decompress(packet, base, N, C):
    return R._add_base(base, decompress(packet, N, C))


# ---- the float64 definition, in the manner of tests/_f64_check.py::check_int4 with 3 levels ----
def check_f64(x, base, pkt, state=None):
    """Packet and error-feedback state against the codec's DEFINITION in float64 (finite inputs), not against the numpy statement above.
    Bounds, derived as _f64_check.py derives int4's: min exact (fp16 compares); scale within 1.5 ulp of (max - min) / (3 + 1e-6); the
    code q = rint(fp16(fp16(d - min) / s)): the quotient is <= 3 (+ the scale's rounding), the rounding of d - min moves it by
    <= 3 * 2^-11, its own rounding by half an ulp of a value below 4, 2^-10 -> |q - clamp((d - min) / s, 0, 3)| <= 0.5 + 0.0025 < 0.503;
    exactly rint, ties to even, where d - min and the quotient are fp16 values as they stand; reconstruction within 0.503 s + ulp16(d) +
    the clamp term on subnormal scales; scale 0: code 3 above the minimum (+inf), 0 at it (0 / 0); state = fp16(base + decode(packet))."""
    import _f64_check as F
    d = F._delta(x, base)
    N, C = d.shape
    qb, s, m = F._split(pkt, [N * C // 4, 2 * C, 2 * C])
    s, m = s.view(F16), m.view(F16)
    q = unpack(qb.reshape(N // 4, C))
    d64, mn, mx = F._minmax_common(d, s, LEVELS + 1, NAME)
    bad = m.astype(F64) != mn
    assert not bad.any(), f"{NAME} min: {int(bad.sum())}/{C} channels differ from the exact column minimum"
    s64 = s.astype(F64)
    with np.errstate(divide="ignore", invalid="ignore"):
        y = np.clip((d64 - mn) / s64, 0, LEVELS)
    y = np.where(s64 == 0, np.where(d64 > mn, float(LEVELS), 0.0), y)
    with np.errstate(divide="ignore", invalid="ignore"):
        F._exact_codes(q, d64 - mn, np.where(s64 > 0, (d64 - mn) / s64, np.nan), 0, LEVELS, NAME)
    err = np.abs(q.astype(F64) - y)
    assert err.max() <= 0.503, f"{NAME} codes: {int((err > 0.503).sum())} further than 0.503 from (d - min) / scale (worst {err.max():.4f})"
    rec = q.astype(F64) * s64 + mn
    bad = np.abs(rec - d64) > 0.503 * s64 + F.ulp16(d64) + F._clamp_term(s64, mn, mx, LEVELS + 1)
    assert not bad.any(), f"{NAME} reconstruction: {int(bad.sum())} elements off d by more than 0.503 scale"
    F._state_equals(state, base, ((q.astype(F16) * s).astype(F16) + m).astype(F16), NAME)
