"""The one allowance in the bit-for-bit packet comparisons (include/cfx.h, INT4 wire layout): where a channel's minimum is zero and zeros of
both signs occur in it, the int4 packet's `min` half may hold either zero - which zero a min reduction keeps depends on the order it meets
them in (numpy: row order; the C oracle: its threads' completion order; a kernel: waves, then row tiles).  Scale, codes, reconstruction and
state do not depend on it: q * s >= +0 and (+0) + (-0) = +0.

    same_packet(name, got, want, x, base, what) -> set of channels whose `min` half differed and was allowed

Everything else - every other codec, every other section of the int4 packet, every other channel - is NF.same_bits: bit for bit (any NaN
equals any NaN).  Callers assert that the returned set lies inside the channels their input planted such zeros in (random inputs: empty)."""
import numpy as np

import _nonfinite as NF

F16, F64 = np.float16, np.float64


def same_packet(name, got, want, x, base, what):
    got = np.asarray(got).view(np.uint16).reshape(-1)
    want = np.asarray(want).view(np.uint16).reshape(-1)
    if name != "int4":
        NF.same_bits(got, want, what)
        return set()
    C = np.asarray(x).shape[-1]
    assert got.size == want.size, (what, got.size, want.size)
    NF.same_bits(got[:-C], want[:-C], what + " (codes, scale)")
    g, w = got[-C:], want[-C:]
    differ = np.flatnonzero((g != w) & ~(((g & 0x7FFF) > 0x7C00) & ((w & 0x7FFF) > 0x7C00)))
    if differ.size == 0:
        return set()
    xs = np.asarray(x).view(F16).reshape(-1, C)[:, differ].astype(F64)
    d = xs.astype(F16) if base is None else (xs - np.asarray(base).view(F16).reshape(-1, C)[:, differ].astype(F64)).astype(F16)
    u = d.view(np.uint16)
    ok = ((g[differ] & 0x7FFF) == 0) & ((w[differ] & 0x7FFF) == 0)                # both halves are zeros
    ok &= d.astype(F64).min(axis=0) == 0                                            # the channel's exact minimum is 0
    ok &= (u == 0).any(axis=0) & (u == 0x8000).any(axis=0)                          # both signs occur among the channel's zeros
    assert ok.all(), f"{what}: int4 min differs on channel(s) {differ[~ok][:8].tolist()} outside the signed-zero rule"
    return set(int(c) for c in differ)
