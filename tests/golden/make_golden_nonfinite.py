#!/usr/bin/env python3
"""G16: the reference's int8 / int4 / top-k codecs on NON-FINITE residuals, captured by IMPORTING the reference in the build
container (see make_golden.py for how).  Data only: inputs (x, base as fp16 bit patterns) and the reference's outputs.

What the reference does there (and the oracles / kernels must do the same):
  * int8 / int4 (compress_quantize.py:452-453, :552-553): torch.min / torch.max over the rows PROPAGATE NaN - one NaN delta in a
    channel makes its min, max, scale NaN, every code of the channel 0 (NaN -> integer) and its reconstruction NaN;
  * top-k (compress_topk.py:82-83): tl.argmax of |x| treats NaN as larger than everything, +inf included, and the FIRST NaN wins.

Inputs (every case is residual: delta = x - base in fp16, inf - inf deltas included):
  mm     (32, 128): a NaN in the middle of a column, NaN in the first / last row of a column, a column holding +inf and -inf,
         a column of alternating +-inf, a column with one +inf, inf - inf (NaN) deltas; int8, int4, and top-k m = 1, 4, 8, 16;
  tk/m{m} (8, 1024): per m, NaN at positions 0, 1, 7, 8, 15 (those < m) of a half-block, two NaNs in one half-block, +inf
         before a NaN, -inf alone, inf - inf in a half-block, NaNs in both lane halves of a 16-wide half-block.

Usage (repo root):  TRITON_INTERPRET=1 TORCHDYNAMO_DISABLE=1 python tests/golden/make_golden_nonfinite.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG          # noqa: E402  (reference import, Store, np16)

NAN, INF = float("nan"), float("inf")
TOPK_M = (1, 4, 8, 16)


def mm_inputs():
    """(32, 128) x, base with the min/max codecs' non-finite cases; finite elsewhere."""
    import torch
    g = torch.Generator().manual_seed(1600)
    N, C = 32, 128
    base = (0.5 * torch.randn((N, C), generator=g)).half()
    x = (base.float() + 0.1 * torch.randn((N, C), generator=g)).half()
    x[13, 3] = NAN                                  # a NaN in the middle of a column
    x[0, 5] = NAN                                   # ... in the first row
    x[N - 1, 6] = NAN                               # ... in the last row
    x[4, 9] = NAN; x[20, 9] = NAN                   # two NaNs in one column
    x[7, 20] = INF; x[25, 20] = -INF                # +inf and -inf in one column
    x[:, 21] = torch.tensor([INF, -INF] * (N // 2), dtype=torch.half)   # a column of +-inf
    x[11, 22] = INF                                 # one +inf: max = inf, min finite
    x[2, 23] = -INF                                 # one -inf
    x[9, 40] = INF; base[9, 40] = INF               # inf - inf = NaN delta
    x[17, 41] = -INF; base[17, 41] = -INF
    x[3, 42] = INF; base[3, 42] = -INF              # inf - (-inf) = +inf delta
    x[30, 127] = NAN                                # the last channel
    return x.contiguous(), base.contiguous()


def tk_inputs(m):
    """(8, 1024) x, base: the top-k half-block cases for 1:m (positions that exist for this m)."""
    import torch
    g = torch.Generator().manual_seed(1610 + m)
    x = (0.5 * torch.randn((8, 1024), generator=g)).half()
    base = (0.5 * torch.randn((8, 1024), generator=g)).half()
    flat_x, flat_b = x.view(-1), base.view(-1)
    hb = [0]                                        # next free half-block

    def take():
        h = hb[0]
        hb[0] += 3                                  # leave untouched half-blocks in between
        return h * m
    for p in (0, 1, 7, 8, 15):                      # NaN at position p of a half-block (8, 15: the upper lane of m = 16)
        if p < m:
            flat_x[take() + p] = NAN
            flat_x[take() + p] = NAN                # (again, in the other half of a block)
    if m >= 2:
        e = take(); flat_x[e + 1] = NAN; flat_x[e + m - 1] = NAN           # two NaNs: the first wins
        e = take(); flat_x[e] = INF; flat_x[e + m - 1] = NAN               # +inf before a NaN: the NaN wins
        e = take(); flat_x[e + m - 1] = INF; flat_x[e] = NAN               # NaN before +inf
        e = take(); flat_x[e + m // 2] = -INF                              # -inf alone
        e = take(); flat_x[e + m - 1] = INF; flat_b[e + m - 1] = INF       # inf - inf
        e = take(); flat_x[e] = -INF; flat_b[e] = -INF; flat_x[e + 1] = 60000.0; flat_b[e + 1] = -60000.0   # NaN delta vs an overflow to inf
    else:
        e = take(); flat_x[e] = INF; flat_b[e] = INF
        e = take(); flat_x[e] = -INF
    if m == 16:
        e = take(); flat_x[e + 7] = NAN; flat_x[e + 8] = NAN               # both lanes of the half-block: the lower lane's NaN
        e = take(); flat_x[e + 9] = NAN; flat_x[e + 3] = INF               # upper lane NaN beats lower lane inf
        e = take(); flat_x[e + 12] = INF; flat_x[e + 15] = NAN             # both in the upper lane
    assert hb[0] * m <= x.numel()
    return x.contiguous(), base.contiguous()


def main():
    MG._import_reference()
    import numpy as np
    from xfuser.compact.compress_quantize import quantize_int8, dequantize_int8, quantize_int4, dequantize_int4
    from xfuser.compact.compress_topk import topk_compress, topk_decompress
    np16 = MG.np16
    st = MG.Store("g16_nonfinite", "x")

    def put_topk(tag, x, base, ms):
        delta = (x - base).contiguous()
        for m in ms:
            val, idx = topk_compress(delta.view(-1, 1024), m)
            st.put(f"{tag}/topk{m}/val", np16(val))
            st.put(f"{tag}/topk{m}/idx", np16(idx))
            st.put(f"{tag}/topk{m}/recon", np16(base + topk_decompress(val, idx, m).view(x.shape)))

    x, base = mm_inputs()
    delta = (x - base).contiguous()
    st.put("mm/x", np16(x))
    st.put("mm/base", np16(base))
    q, s, z = quantize_int8(delta)
    st.put("mm/int8/q", np16(q)); st.put("mm/int8/scale", np16(s)); st.put("mm/int8/zp", np16(z))
    st.put("mm/int8/recon", np16(base + dequantize_int8(q, s, z)))
    q, s, mn = quantize_int4(delta)
    st.put("mm/int4/q", np16(q)); st.put("mm/int4/scale", np16(s)); st.put("mm/int4/min", np16(mn))
    st.put("mm/int4/recon", np16(base + dequantize_int4(q, s, mn)))
    put_topk("mm", x, base, TOPK_M)
    for m in TOPK_M:
        x, base = tk_inputs(m)
        st.put(f"tk/m{m}/x", np16(x))
        st.put(f"tk/m{m}/base", np16(base))
        put_topk(f"tk/m{m}", x, base, (m,))
    fn = "g16_nonfinite.npz"
    np.savez_compressed(os.path.join(HERE, fn), **st.arrays)
    man_path = os.path.join(HERE, "MANIFEST.json")
    with open(man_path) as f:
        man = json.load(f)
    man[fn] = st.manifest
    with open(man_path, "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)
    print("wrote", fn, len(st.arrays), "arrays")


if __name__ == "__main__":
    main()
