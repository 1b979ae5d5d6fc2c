"""Shapes, values and planted errors of the tests of the native attention forward at the head dims BETWEEN 64 and 128
(cfx_attn_fwd_blocks_hd: D = 72, 80, .. 120; tests/test_attn_hd_f64.py on the CPU, tests/test_gpu_attn_hd.py on the GPU).

A case is a dict for `_attn_var_cases.build`, which is generic in D: id, B, Sq, sks, H, D, kind (+ the kind's parameters).  H = 3, so that
a head's rows do not start on 256-byte boundaries (3 x 72 x 2 = 432 bytes a key).  The witness and the bound are tests/_attn_var_f64.py's
with the TRUE D: what the launch adds past D are exact zeros, which round nothing - no new constant.

The planted errors are the ones a walk in 16-column k-steps and 32-row accumulator blocks over a D that is a multiple of neither can make
and the 64 / 128 forms cannot, in float64:
  droptail     the scores over the first 16 floor(D / 16) columns only (the last, partial k-step lost)
  dropblock    out's columns at or past 32 floor(D / 32) returned as 0 (the last, partial accumulator block lost)
  headstride   head h of K read at element h 16 ceil(D / 16) of a key's row instead of h D (the padded width taken for the pitch); what lies
               past the block's end reads as zeros
"""
import numpy as np

import _attn_f64 as W
import _attn_var_cases as V

DIMS = (72, 80, 88, 96, 104, 112, 120)
H = 3
LENGTHS = ([1], [65, 64, 63], [100, 37, 128, 5], list(range(1, 17)), [64, 128, 192])
SQS = (1, 33, 129)
PLANTS = ("droptail", "dropblock", "headstride")


def _cases():
    out = []

    def add(Sq, sks, B, D, kind, **kw):
        tag = "".join(f"-{k}{v}" for k, v in kw.items())
        out.append(dict(B=B, Sq=Sq, sks=list(sks), H=H, D=D, kind=kind, id=f"{kind}{tag}-q{Sq}-{V._tag(list(sks))}-b{B}-d{D}", **kw))
    for di, D in enumerate(DIMS):
        for i, sks in enumerate(LENGTHS):                            # every D x every length list: gaussian; Sq and B rotate
            add(SQS[(i + di) % 3], sks, 1 + (i + di) % 2, D, "gauss")
        add(SQS[di % 3], [65, 64, 63], 2 - di % 2, D, "peak", pblk=di % 3, pend="last")          # the designated key in a full tile, a tail ...
        add(SQS[(di + 1) % 3], [100, 37, 128, 5], 1 + di % 2, D, "peak", pblk=3 - di % 4, pend="first")
    for D, sks, Sq, B in ((72, [65, 64, 63], 33, 2), (88, [100, 37, 128, 5], 129, 1), (120, list(range(1, 17)), 33, 2)):
        add(Sq, sks, B, D, "ramp")
    return out


CASES = _cases()


def can_show(plant, case):
    """Whether the case can show the planted error - decided from the case alone.  gauss only: every key weighs about 1 / K of a row and
    every column of q, k, v counts alike.  (ramp: the 1e4 scores' own rounding makes the bound as large as what 8 lost columns move;
    peak: the designated key's score sits in column 0 and its weight > 0.9 hides the rest.)  The D decides the rest: a D that is a
    multiple of 16 has no partial k-step and no padded width, a multiple of 32 no partial accumulator block."""
    if case["kind"] != "gauss":
        return False
    if plant in ("droptail", "headstride"):
        return case["D"] % 16 != 0
    if plant == "dropblock":
        return case["D"] % 32 != 0
    raise KeyError(plant)


def _restride(k, pitch):
    """k (B, n, H, D) as a kernel reads it that takes head h at element h * pitch of a key's row: flat memory, zeros past the end"""
    B, n, Hh, D = k.shape
    flat = np.concatenate([k.reshape(-1), np.zeros(Hh * pitch + D, k.dtype)])
    idx = (np.arange(B * n)[:, None, None] * (Hh * D) + np.arange(Hh)[None, :, None] * pitch + np.arange(D)[None, None, :])
    return flat[idx].reshape(B, n, Hh, D)


def planted(plant, q, ks, vs, scale):
    """(out, lse) of the witness's arithmetic with one error planted"""
    D = q.shape[-1]
    if plant == "droptail":
        c = 16 * (D // 16)
        s, _ = W.scores(q[..., :c], [k[..., :c] for k in ks], scale)
        m = s.max(-1, keepdims=True)
        p = np.exp(s - m)
        L = p.sum(-1, keepdims=True)
        vd = np.concatenate([v.astype(np.float64) for v in vs], axis=1).transpose(0, 2, 1, 3)
        return ((p / L) @ vd).transpose(0, 2, 1, 3), (m + np.log(L))[..., 0].transpose(0, 2, 1)
    if plant == "dropblock":
        out, lse = W.witness(q, ks, vs, scale)
        out = out.copy()
        out[..., 32 * (D // 32):] = 0.0
        return out, lse
    if plant == "headstride":
        return W.witness(q, [_restride(k, 16 * ((D + 15) // 16)) for k in ks], vs, scale)
    raise KeyError(plant)
