"""Every codec's packet and error-feedback state checked against the codec's DEFINITION, computed in float64 - not against the oracle.
check(name, param, x, base, packet_words, state) raises AssertionError naming what is wrong.  Finite inputs only.

d = fp16(x - base) is formed exactly (float64 difference of two fp16 values, rounded once to fp16 = the fp16 subtraction).
fp16 ulp(v) = 2^(floor(log2|v|) - 10) (2^-24 below 2^-14).  Each fp16 rounding moves a value by <= 2^-11 relative (half an ulp).

Bounds (each derived in its own line):
  1-bit / 2-bit  V[c], row means: fp16(fp32(exact sum) / n): two fp32 roundings (2^-24 each) + one fp16 rounding -> <= 1 ulp.
                 U = fp16(rowmean / mean(rowmean)): rowmean 2^-11, mean(rowmean) 2^-11 + its own 2^-11, quotient 2^-11 -> <= 4 * 2^-11
                 relative < 4 ulp (2-bit tok: the + 1e-6 of the reference adds 1e-6 / mean to the relative error).
                 sign bit == (d >= 0) exactly; 2-bit magnitude bit == |d| > fp16(chan * tok) exactly (the packet's own scales), and
                 consistent with the float64 threshold colmean * rowmean / mean(rowmean) wherever |d| is outside 5 * 2^-11 of it.
  int8 / int4    per-channel min / max: exact (fp16 compares).  scale = fp16(fp16(max - min) / (levels - 1 + 1e-6)): the difference
                 2^-11 relative + the quotient's rounding 0.5 ulp -> < 1.5 ulp.
                 int8 code q = rint(fp16(fp16(d / s) + zp)): |d / s| <= 2^8 there, each of the two roundings <= 0.125 ->
                 |q - clamp(d / s + zp)| <= 0.75 (0.5 for rint).  int4 code q = rint(fp16(fp16(d - min) / s)): the two roundings
                 <= 15 * 2^-11 + 2^-8 < 0.02 -> |q - clamp((d - min) / s)| <= 0.52.  Reconstruction error |decode - d| <= the code bound
                 times s (the decode evaluated in float64 from the packet; int8: where the zero point is not clamped).
                 The clamp term.  The code bound is about clamp(.): an element whose quotient lies above the top code L = levels - 1 (15,
                 255) takes L, and its reconstruction then falls short of d by (d - min) - L * s <= (max - min) - L * s, which is
                 positive whenever the packet's scale s was rounded BELOW (max - min) / L.  With r = (max - min) / (L + 1e-6), the
                 quantity the scale check above compares s with: (max - min) - L * s = L * (r - s) + 1e-6 * r <= L * |s - r| + 1e-6 * r.
                 A normal s is within 1.5 * 2^-11 * s of r, the loss within L * 1.5 * 2^-11 * s of a code (the 0.52 / 0.75 and ulp16(d)
                 hold it); a subnormal s is a whole number of units of 2^-24 and can be half a unit from r, so the loss reaches L / 2
                 units - several ulp16(d).  So on channels whose packet scale is below 2^-14, and only there, the reconstruction bound
                 grows by L * |s - r| (the 1e-6 * r left over is < 2^-14 * 16 * 1e-6 < 2^-33, far inside the ulp16(d) >= 2^-24 already
                 there).  int8: the same with the top code 127 = zp + 255 where the zero point is -128, fewer levels above zero otherwise
                 (a smaller loss: the term is an upper bound).
                 Exact quotients.  Where every intermediate of the code's arithmetic is an fp16 value as it stands (int4: d - min and
                 (d - min) / s; int8: d / s and d / s + zp) no rounding happens before rint, and the code is rint of that value, ties to
                 even - exactly, not within a bound.
                 Scale 0 under a non-zero range (a range of one unit): the int4 quotient is +inf above the minimum (code 15) and 0 / 0
                 at it (NaN -> code 0); every code reconstructs as min, within the one unit of d.
  top-k          the kept index is the FIRST argmax of |d| in its half-block, the kept value is d there bit for bit, every other element
                 of the state equals base (and the kept one equals fp16(base + d)).
States: the error-feedback state must also equal fp16(base + decode(packet)) bit for bit, decode in fp16 as the codec defines it.
"""
import numpy as np

F16, F64 = np.float16, np.float64


def ulp16(v):
    v = np.abs(np.asarray(v, dtype=F64))
    e = np.floor(np.log2(np.maximum(v, 2.0 ** -14)))
    return np.exp2(e - 10)


def _within_ulps(got16, want64, k, what):
    got = np.asarray(got16).view(F16).astype(F64).reshape(-1)
    want = np.asarray(want64, dtype=F64).reshape(-1)
    assert np.isfinite(got).all(), f"{what}: non-finite value"
    err = np.abs(got - want) / ulp16(want)
    bad = err > k
    assert not bad.any(), f"{what}: {int(bad.sum())}/{got.size} beyond {k} ulp (worst {err.max():.2f} at {int(np.argmax(err))})"


def _delta(x, base):
    x = np.asarray(x).view(F16)
    if base is None:
        return x.copy()
    return (x.astype(F64) - np.asarray(base).view(F16).astype(F64)).astype(F16)


def _state_equals(state, base, recv16, what):
    if state is None:
        return
    want = recv16 if base is None else (np.asarray(base).view(F16) + recv16).astype(F16)
    got = np.asarray(state).view(np.uint16).reshape(want.shape)
    bad = got != want.view(np.uint16)
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.size} state elements differ from fp16(base + decode(packet))"


def _absmean_stats64(d):
    a = np.abs(d.astype(F64))
    col, row = a.mean(axis=0), a.mean(axis=1)
    return col, row, row.mean()


def _split(words, sizes_bytes):
    b = np.ascontiguousarray(np.asarray(words).view(np.uint16).reshape(-1)).view(np.uint8)
    out, o = [], 0
    for s in sizes_bytes:
        out.append(b[o:o + s])
        o += s
    assert o == b.size, f"packet is {b.size} bytes, the layout {o}"
    return out


def check_binary(x, base, pkt, state):
    d = _delta(x, base)
    N, C = d.shape
    bits, U, V = _split(pkt, [N * C // 8, 2 * N, 2 * C])
    U, V = U.view(F16), V.view(F16)
    col, row, mu = _absmean_stats64(d)
    _within_ulps(V, col, 1, "1-bit V (column means of |d|)")
    _within_ulps(U, row / mu, 4, "1-bit U (row mean / mean of row means)")
    sign = ((bits.reshape(N, C // 8)[:, :, None] >> np.arange(8, dtype=np.uint8)) & 1).reshape(N, C).astype(bool)
    bad = sign != (d >= 0)
    assert not bad.any(), f"1-bit sign bits: {int(bad.sum())}/{d.size} differ from d >= 0"
    mag = (U.reshape(-1, 1) * V.reshape(1, -1)).astype(F16)
    _state_equals(state, base, np.where(sign, mag, -mag).astype(F16), "1-bit")


def check_int2(x, base, pkt, state):
    d = _delta(x, base)
    N, C = d.shape
    codes, tok, chan = _split(pkt, [N * C // 4, 2 * N, 2 * C])
    tok, chan = tok.view(F16), chan.view(F16)
    col, row, mu = _absmean_stats64(d)
    _within_ulps(chan, col, 1, "2-bit chan (column means of |d|)")
    _within_ulps(tok, row / (mu + 1e-6), 4, "2-bit tok (row mean / (mean of row means + 1e-6))")
    idx = ((codes.reshape(N, C // 4)[:, :, None] >> (2 * np.arange(4, dtype=np.uint8))) & 3).reshape(N, C)
    bad = (idx >> 1).astype(bool) != (d >= 0)
    assert not bad.any(), f"2-bit sign bits: {int(bad.sum())}/{d.size} differ from d >= 0"
    thr = (chan.reshape(1, -1) * tok.reshape(-1, 1)).astype(F16)
    big = (idx & 1).astype(bool)
    bad = big != (np.abs(d) > thr)
    assert not bad.any(), f"2-bit magnitude bits: {int(bad.sum())}/{d.size} differ from |d| > fp16(chan * tok)"
    thr64 = col.reshape(1, -1) * (row / mu).reshape(-1, 1)
    ad = np.abs(d.astype(F64))
    clear = np.abs(ad - thr64) > 5 * 2.0 ** -11 * thr64 + 2.0 ** -24
    bad = clear & (big != (ad > thr64))
    assert not bad.any(), f"2-bit magnitude bits: {int(bad.sum())} contradict the float64 threshold"
    small, large = (F16(0.5) * thr).astype(F16), (F16(2.0) * thr).astype(F16)
    lvl = np.where(big, large, small)
    _state_equals(state, base, np.where(idx >> 1, lvl, -lvl).astype(F16), "2-bit")


def _minmax_common(d, scale, levels, what):
    d64 = d.astype(F64)
    mn, mx = d64.min(axis=0), d64.max(axis=0)
    _within_ulps(scale, (mx - mn) / (levels - 1 + 1e-6), 1.5, f"{what} scale")
    return d64, mn, mx


def _clamp_term(s64, mn, mx, levels):
    """(levels - 1) * |s - (max - min) / (levels - 1 + 1e-6)| on channels whose packet scale is subnormal, 0 elsewhere (module docstring)"""
    return np.where(s64 < 2.0 ** -14, (levels - 1) * np.abs(s64 - (mx - mn) / (levels - 1 + 1e-6)), 0.0)


def _is_f16(v):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.isfinite(v) & (v.astype(F16).astype(F64) == v)


def _exact_codes(q, a, t, lo, hi, what):
    """the code's arithmetic is rint(fp16(t)), t formed from fp16(a) in one operation (int8: a = d / s, t = a + zp; int4: a = d - min,
    t = a / s).  Where a and t are fp16 values as they stand, the code is clip(rint(t)), ties to even, exactly."""
    exact = _is_f16(a) & _is_f16(t)
    want = np.clip(np.rint(np.where(exact, t, 0.0)), lo, hi)
    bad = exact & (q.astype(F64) != want)
    assert not bad.any(), (f"{what} exact quotients: {int(bad.sum())}/{int(exact.sum())} codes differ from rint (ties to even) of an exactly "
                           "representable quotient")


def check_int8(x, base, pkt, state):
    d = _delta(x, base)
    N, C = d.shape
    q, s, zp = _split(pkt, [N * C, 2 * C, 2 * C])
    q, s, zp = q.view(np.int8).reshape(N, C), s.view(F16), zp.view(np.int16)
    d64, mn, mx = _minmax_common(d, s, 256, "int8")
    s64, z64 = s.astype(F64), zp.astype(F64)
    live = s64 > 0                  # a constant channel (max == min, e.g. N == 1) has scale 0: it reconstructs as 0 (the state check)
    with np.errstate(divide="ignore", invalid="ignore"):
        want_z = np.clip(-128.0 - np.round(mn / s64), -128, 127)
        y = np.clip(d64 / s64 + z64, -128, 127)
    assert np.all(np.abs(z64 - want_z)[live] <= 1), "int8 zero point further than 1 from -128 - round(min / scale)"
    with np.errstate(divide="ignore", invalid="ignore"):
        _exact_codes(q, np.where(live, d64 / s64, np.nan), np.where(live, d64 / s64 + z64, np.nan), -128, 127, "int8")
    err = np.where(live, np.abs(q.astype(F64) - y), 0.0)
    assert err.max() <= 0.75, f"int8 codes: {int((err > 0.75).sum())} further than 0.75 from d / scale + zp (worst {err.max():.3f})"
    rec = (q.astype(F64) - z64) * s64
    lim = 0.75 * s64 + ulp16(d64) + _clamp_term(s64, mn, mx, 256)
    # (only where the zero point is not clamped: with the min far from 0 relative to the range - few rows - the reference's int16 zero
    # point saturates at -128 / 127 and the codes clamp, the code bound above still holds)
    unclamped = live & (np.abs(-128.0 - np.round(np.where(live, mn / np.where(live, s64, 1), 0)) + 0.5) < 127.5)
    bad = (np.abs(rec - d64) > lim) & unclamped
    assert not bad.any(), f"int8 reconstruction: {int(bad.sum())} elements off d by more than 0.75 scale"
    t = (q.astype(F16) - zp.astype(F16)).astype(F16)
    _state_equals(state, base, (t * s).astype(F16), "int8")


def check_int4(x, base, pkt, state):
    d = _delta(x, base)
    N, C = d.shape
    qb, s, m = _split(pkt, [N * C // 2, 2 * C, 2 * C])
    s, m = s.view(F16), m.view(F16)
    qb = qb.reshape(N // 2, C)
    q = np.empty((N, C), np.uint8)
    q[0::2], q[1::2] = qb & 15, qb >> 4
    d64, mn, mx = _minmax_common(d, s, 16, "int4")
    bad = m.astype(F64) != mn
    assert not bad.any(), f"int4 min: {int(bad.sum())}/{C} channels differ from the exact column minimum"
    s64 = s.astype(F64)
    with np.errstate(divide="ignore", invalid="ignore"):
        y = np.clip((d64 - mn) / s64, 0, 15)
    y = np.where(s64 == 0, np.where(d64 > mn, 15.0, 0.0), y)       # scale 0: +inf above the minimum, 0 / 0 -> 0 at it
    with np.errstate(divide="ignore", invalid="ignore"):
        _exact_codes(q, d64 - mn, np.where(s64 > 0, (d64 - mn) / s64, np.nan), 0, 15, "int4")
    err = np.abs(q.astype(F64) - y)
    assert err.max() <= 0.52, f"int4 codes: {int((err > 0.52).sum())} further than 0.52 from (d - min) / scale (worst {err.max():.3f})"
    rec = q.astype(F64) * s64 + mn
    bad = np.abs(rec - d64) > 0.52 * s64 + ulp16(d64) + _clamp_term(s64, mn, mx, 16)
    assert not bad.any(), f"int4 reconstruction: {int(bad.sum())} elements off d by more than 0.52 scale"
    _state_equals(state, base, ((q.astype(F16) * s).astype(F16) + m).astype(F16), "int4")


def check_topk(x, base, pkt, state, m):
    d = _delta(x, base)
    N, C = d.shape
    E = N * C
    val, idx = _split(pkt, [2 * E // m, E // (2 * m)])
    val = val.view(np.uint16).reshape(-1, 2)
    hb = np.abs(d.reshape(-1, 2, m).astype(F64))
    want = np.argmax(hb, axis=-1)                               # numpy: the first maximum
    sel = np.stack([idx >> 4, idx & 15], axis=-1).astype(np.int64)
    bad = sel != want
    assert not bad.any(), f"top-k 1:{m} indices: {int(bad.sum())}/{sel.size} half-blocks keep another element than the first argmax |d|"
    dv = np.take_along_axis(d.reshape(-1, 2, m).view(np.uint16), want[..., None], axis=-1)[..., 0]
    bad = val != dv
    assert not bad.any(), f"top-k 1:{m} values: {int(bad.sum())} differ from d at the kept index"
    recv = np.zeros((E // (2 * m), 2, m), F16)
    np.put_along_axis(recv, want[..., None], dv.view(F16)[..., None], axis=-1)
    _state_equals(state, base, recv.reshape(N, C), f"top-k 1:{m}")


def check(name, param, x, base, pkt, state=None):
    if name == "topk":
        return check_topk(x, base, pkt, state, param)
    return {"binary": check_binary, "int2": check_int2, "int4": check_int4, "int8": check_int8}[name](x, base, pkt, state)
