"""Shapes and values of the tests of the native attention forward over K,V blocks of UNEQUAL length (cfx_attn_fwd_blocks_var;
tests/test_attn_var_f64.py on the CPU, tests/test_gpu_attn_var.py on the GPU): the smallest length lists that reach every index path of a
walk whose tiles per block, batch stride and key mask are per block, and the values that make an index slip visible.

A case is a dict: id, B, Sq, sks (the blocks' key counts), H, D, kind (+ the kind's parameters).  `build(case, dtype)` returns
(q, ks, vs, scale) as float32 numpy arrays of exactly representable values of the element type, ks[i] / vs[i] (B, sks[i], H, D).

kinds (values as tests/_attn_cases.py makes them: A0, RAMP and to_elem are its own)
  gauss    q, k, v standard normal
  peak     gauss, q[..., 0] = A0 and ONE designated key - block `pblk`, its first or its last key (`pend`) - with a score of 16 and a V row
           of its own: more than 0.9 of every row's weight
  ramp     gauss, q[..., 0] = A0 and block b's keys shifted by RAMP[b] e_0: block maxima rising and falling by up to 1e4
"""
import zlib

import numpy as np

import _attn_cases as C

LENGTHS = (
    [1],
    [64, 1],
    [1, 64],
    [65, 64, 63],
    [16, 64, 64, 64],                  # a front joint block shorter than the shards
    [64, 64, 64, 16],                  # ... a rear one
    [130, 40, 40],                     # a joint block longer than the shards
    [100, 37, 128, 5],
    list(range(1, 17)),                # sixteen blocks
    [64, 128, 192],
)
SQS = (1, 33, 80, 129)
PEAK_LISTS = ([64, 1], [1, 64], [65, 64, 63], [130, 40, 40], [100, 37, 128, 5])
RAMP_LISTS = ([65, 64, 63], [16, 64, 64, 64], [64, 64, 64, 16], [100, 37, 128, 5], list(range(1, 17)))


def _tag(sks):
    return "k" + ("1to16" if sks == list(range(1, 17)) else "_".join(map(str, sks)))


def _cases():
    out = []

    def add(Sq, sks, B, D, kind, **kw):
        tag = "".join(f"-{k}{v}" for k, v in kw.items())
        out.append(dict(B=B, Sq=Sq, sks=list(sks), H=2, D=D, kind=kind, id=f"{kind}{tag}-q{Sq}-{_tag(list(sks))}-b{B}-d{D}", **kw))
    for i, sks in enumerate(LENGTHS):                                # every length list, every Sq: gaussian; B = 2 on every list but three
        add(SQS[i % 4], sks, 1 if i in (0, 4, 9) else 2, 64, "gauss")
    for i, sks in enumerate(([65, 64, 63], [130, 40, 40], [100, 37, 128, 5], [64, 128, 192])):      # the handful at D = 128
        add(SQS[(i + 1) % 4], sks, 2 - i % 2, 128, "gauss")
    i = 0
    for sks in PEAK_LISTS:                                           # the designated key at the first and the last key of every block in turn
        for blk, n in enumerate(sks):
            for end in ("first", "last")[:1 if n == 1 else 2]:
                add(SQS[i % 4], sks, 2 - (i % 3 == 0), 64, "peak", pblk=blk, pend=end)
                i += 1
    add(33, [100, 37, 128, 5], 2, 128, "peak", pblk=1, pend="last")
    for i, sks in enumerate(RAMP_LISTS):
        add(SQS[(i + 2) % 4], sks, 1 + i % 2, 64, "ramp")
    add(80, [65, 64, 63], 2, 128, "ramp")
    return out


CASES = _cases()


def peak_position(case):
    """(block, key) of the designated key of a `peak` case"""
    return case["pblk"], 0 if case["pend"] == "first" else case["sks"][case["pblk"]] - 1


def build(case, dtype):
    B, Sq, sks, H, D, kind = (case[k] for k in ("B", "Sq", "sks", "H", "D", "kind"))
    rng = np.random.default_rng(zlib.crc32((case["id"] + dtype).encode()))
    scale = float(np.float32(D ** -0.5))
    q = rng.standard_normal((B, Sq, H, D))
    ks = [rng.standard_normal((B, n, H, D)) for n in sks]
    vs = [rng.standard_normal((B, n, H, D)) for n in sks]
    if kind == "peak":
        blk, key = peak_position(case)
        q[..., 0] = C.A0
        ks[blk][:, key] = 0.0
        ks[blk][:, key, :, 0] = 16.0 / (scale * C.A0)               # its score is 16 for every row; the others' are ~N(0, 1.x)
        vs[blk][:, key] = 2.0 + (np.arange(D) % 7) / 4.0
    elif kind == "ramp":
        q[..., 0] = C.A0
        for b_ in range(len(sks)):
            ks[b_][..., 0] = ks[b_][..., 0] * 0.25 + C.RAMP[b_] / (scale * C.A0)
    return C.to_elem(q, dtype), [C.to_elem(k, dtype) for k in ks], [C.to_elem(v, dtype) for v in vs], scale
