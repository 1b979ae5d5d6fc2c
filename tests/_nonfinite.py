"""Golden G16 (tests/golden/make_golden_nonfinite.py): the reference's int8 / int4 / top-k codecs on residuals with NaN and +-inf,
as (id, codec, param, x, base, packet words, reconstruction) - the packet in the C-ABI's wire layout (oracle/ref_np.py compress).

1-bit and 2-bit are not here: their outputs on non-finite input are unspecified (include/cfx.h)."""
import numpy as np

import _golden as G

FN = "g16_nonfinite.npz"
TOPK_M = (1, 4, 8, 16)


def _words(*parts):
    return np.concatenate([np.ascontiguousarray(p).reshape(-1).view(np.uint8) for p in parts]).view(np.uint16)


def cases():
    g = lambda k: G.get(FN, k)          # noqa: E731
    out = []
    x, b = g("mm/x"), g("mm/base")
    out.append(("mm-int8", "int8", 0, x, b, _words(g("mm/int8/q"), g("mm/int8/scale"), g("mm/int8/zp")), g("mm/int8/recon")))
    out.append(("mm-int4", "int4", 0, x, b, _words(g("mm/int4/q"), g("mm/int4/scale"), g("mm/int4/min")), g("mm/int4/recon")))
    for m in TOPK_M:
        out.append((f"mm-topk{m}", "topk", m, x, b, _words(g(f"mm/topk{m}/val"), g(f"mm/topk{m}/idx")), g(f"mm/topk{m}/recon")))
    for m in TOPK_M:
        t = f"tk/m{m}"
        out.append((f"tk-topk{m}", "topk", m, g(f"{t}/x"), g(f"{t}/base"), _words(g(f"{t}/topk{m}/val"), g(f"{t}/topk{m}/idx")),
                    g(f"{t}/topk{m}/recon")))
    return out


def ids():
    return [c[0] for c in cases()]


def same_bits(a, b, what):
    """bit for bit, except that any NaN equals any NaN (payload and sign of a NaN are not specified)."""
    a = np.asarray(a).view(np.uint16).reshape(-1)
    b = np.asarray(b).view(np.uint16).reshape(-1)
    assert a.size == b.size, (what, a.size, b.size)
    ok = (a == b) | (((a & 0x7fff) > 0x7c00) & ((b & 0x7fff) > 0x7c00))
    assert ok.all(), f"{what}: {int((~ok).sum())}/{a.size} halves differ (first at {int(np.argmax(~ok))})"
