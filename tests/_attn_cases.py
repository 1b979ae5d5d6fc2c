"""Shapes and values of the native attention forward's tests (cfx_attn_fwd_blocks; tests/test_attn_fwd_f64.py on the CPU,
tests/test_gpu_attn_fwd.py on the GPU): the smallest shapes that reach every index path of a kernel that walks n blocks of Sk keys
in 64-key tiles (32-key half tiles) for 32-row query groups, and the values that make an index slip visible.

A case is a dict: id, B, Sq, Sk, n, H, D, kind (+ the kind's parameters).  `build(case, dtype)` returns (q, ks, vs, scale) as float32
numpy arrays that hold exactly representable values of the element type ("fp16" / "bf16"), q (B, Sq, H, D), ks[i] / vs[i] (B, Sk, H, D).

kinds
  gauss    q, k, v standard normal
  int      q, k small integers (every score's fp32 sum is exact), v normal: the single-key case is held bit for bit
  peak     gauss, but q[..., 0] = A and ONE designated key (block, key) = BIG e_0 with a V row of its own: it carries more than 0.9 of
           every row's weight, so a kernel that loses, doubles or misplaces exactly that key is off by the order of the values
  ramp     gauss, q[..., 0] = A and block b's keys shifted by c_b e_0: the blocks' score maxima rise and fall by up to 1e4 from block to
           block (every rescale direction, old sums flushed to zero and not), scores reach +-1e4
  vmax     gauss scores, v = +-65504 (fp16) / +-2^100 (bf16)
  zeroq    q = 0: all scores 0 whatever the scale
  equal    q and every key constant vectors: all scores equal and non-zero
"""
import zlib

import numpy as np

SQS = (1, 31, 32, 33, 65, 130, 257)
SKS = (1, 63, 64, 65, 100)
NS = (1, 2, 3, 8, 16)
A0 = 4.0                    # q[..., 0] of the peak / ramp kinds


def to_elem(x, dtype):
    """float array -> the nearest (even) value of the element type, as float32"""
    x = np.asarray(x, dtype=np.float32)
    if dtype == "fp16":
        return x.astype(np.float16).astype(np.float32)
    b = x.view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


def _cases():
    out = []

    def add(Sq, Sk, n, H, B, D, kind, **kw):
        tag = "".join(f"-{k}{v}" for k, v in kw.items())
        out.append(dict(B=B, Sq=Sq, Sk=Sk, n=n, H=H, D=D, kind=kind, id=f"{kind}{tag}-q{Sq}-k{Sk}-n{n}-h{H}-b{B}-d{D}", **kw))
    # every Sq x one Sk each, every Sk x one Sq each, every n: gaussian
    for i, Sq in enumerate(SQS):
        add(Sq, SKS[i % 5], NS[i % 5], (1, 3)[i % 2], (1, 2)[(i // 2) % 2], (64, 128)[i % 2], "gauss")
    for i, Sk in enumerate(SKS):
        add(SQS[(i + 3) % 7], Sk, NS[(i + 2) % 5], (3, 1)[i % 2], (2, 1)[i % 2], (128, 64)[i % 2], "gauss")
    add(33, 100, 16, 3, 2, 128, "gauss")            # 1600 keys a row: the longest walk
    add(257, 65, 16, 1, 1, 64, "gauss")
    # the single key, and single blocks
    add(1, 1, 1, 1, 1, 64, "int")
    add(33, 1, 1, 3, 2, 128, "int")
    add(65, 64, 1, 1, 1, 128, "int")
    # a designated key at every place an index can slip: (block, key) as "where"
    for i, (Sk, n, where) in enumerate([(100, 3, "tile_first"), (100, 3, "tile_last"), (100, 2, "block_last"), (65, 3, "tail"), (100, 2, "tail"),
                                        (64, 8, "lastblock_first"), (63, 16, "lastblock_first"), (65, 2, "block_last"), (1, 8, "lastblock_first"),
                                        (64, 2, "tile_last")]):
        add(SQS[(i + 1) % 7], Sk, n, (1, 3)[i % 2], (2, 1)[i % 2], (64, 128)[i % 2], "peak", where=where)
    # block maxima rising and falling, scores to +-1e4
    for i, (Sk, n) in enumerate([(65, 8), (100, 3), (64, 16), (1, 8), (63, 2)]):
        add(SQS[(i + 2) % 7], Sk, n, (3, 1)[i % 2], (1, 2)[i % 2], (128, 64)[i % 2], "ramp")
    # values at the top of the type's range
    add(33, 65, 3, 3, 1, 64, "vmax")
    add(130, 100, 8, 1, 2, 128, "vmax")
    add(31, 63, 2, 1, 1, 128, "vmax")
    # degenerate scores
    add(33, 65, 3, 1, 1, 64, "zeroq")
    add(65, 100, 2, 3, 1, 128, "zeroq")
    add(33, 65, 3, 1, 2, 128, "equal")
    add(130, 63, 8, 3, 1, 64, "equal")
    return out


CASES = _cases()
FLUX = dict(B=1, Sq=544, Sk=544, n=8, H=24, D=128, kind="gauss", id="flux-gauss-q544-k544-n8-h24-b1-d128")


def peak_position(case):
    """(block, key) of the designated key of a `peak` case"""
    Sk, n, w = case["Sk"], case["n"], case["where"]
    if w == "tile_first":
        return (1 % n, 64 if Sk > 64 else 0)
    if w == "tile_last":
        return (0, 63 if Sk >= 64 else Sk - 1)
    if w == "block_last":
        return (0, Sk - 1)
    if w == "tail":
        assert Sk > 64
        return (n - 1, 64 + (Sk - 65) // 2)
    assert w == "lastblock_first"
    return (n - 1, 0)


RAMP = (0.0, 30.0, 1.0e4, -1.0e4, 5.0, 9990.0, 9999.0, -3.0, 4000.0, 4100.0, 4090.0, -9000.0, 9000.0, 0.0, 1.0e4, 1.0e4 - 20.0)   # score offset of block b


def build(case, dtype):
    B, Sq, Sk, n, H, D, kind = (case[k] for k in ("B", "Sq", "Sk", "n", "H", "D", "kind"))
    rng = np.random.default_rng(zlib.crc32((case["id"] + dtype).encode()))
    scale = float(np.float32(D ** -0.5))
    q = rng.standard_normal((B, Sq, H, D))
    ks = [rng.standard_normal((B, Sk, H, D)) for _ in range(n)]
    vs = [rng.standard_normal((B, Sk, H, D)) for _ in range(n)]
    if kind == "int":
        q = rng.integers(-3, 4, (B, Sq, H, D)).astype(np.float64)
        ks = [rng.integers(-3, 4, (B, Sk, H, D)).astype(np.float64) for _ in range(n)]
    elif kind == "peak":
        blk, key = peak_position(case)
        q[..., 0] = A0
        ks[blk][:, key] = 0.0
        ks[blk][:, key, :, 0] = 16.0 / (scale * A0)                 # its score is 16 for every row; the others' are ~N(0.25, 1.x)
        vs[blk][:, key] = 2.0 + (np.arange(D) % 7) / 4.0
    elif kind == "ramp":
        q[..., 0] = A0
        for b_ in range(n):
            ks[b_][..., 0] = ks[b_][..., 0] * 0.25 + RAMP[b_] / (scale * A0)
    elif kind == "vmax":
        top = 65504.0 if dtype == "fp16" else 2.0 ** 100
        vs = [np.where(rng.random((B, Sk, H, D)) < 0.5, -top, top) for _ in range(n)]
    elif kind == "zeroq":
        q = np.zeros_like(q)
    elif kind == "equal":
        q = np.full_like(q, 0.5)
        ks = [np.full_like(k, 0.25) for k in ks]
    return to_elem(q, dtype), [to_elem(k, dtype) for k in ks], [to_elem(v, dtype) for v in vs], scale
