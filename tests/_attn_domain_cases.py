"""Cases that hold the three one-launch attention entry points - cfx_attn_fwd_blocks ("eq"), cfx_attn_fwd_blocks_var ("var") and
cfx_attn_fwd_blocks_hd ("hd") - to the parts of include/cfx.h's contract the other case modules leave alone: a softmax scale that is NOT
D ** -0.5, the value kinds `vmax`, `zeroq`, `equal` and `int` on the two unequal-length walks, and query counts that are whole query
tiles.  tests/test_attn_domain_f64.py (CPU) and tests/test_gpu_attn_domain.py (GPU) run them.

A case is a dict for the existing `build` functions - `_attn_cases.build` for "eq" (id, B, Sq, Sk, n, H, D, kind), `_attn_var_cases.build`
for "var" and "hd" (id, B, Sq, sks, H, D, kind) - plus
  ep       the entry point: "eq", "var", "hd"
  group    "scale", "kind", "int" or "sq": why the case is here
  sname    the scale's name (SCALE_NAMES, "def" = fp32(D ** -0.5), "sub" = 2^-149) and  scale  its value, a float that IS an fp32 value
  dtypes   the element types the case runs in (both unless stated)
`build(case, dtype)` returns (q, ks, vs, scale) as the existing builders do, float32 arrays of exactly representable values of the element
type, with `build`'s own scale REPLACED by the case's and nothing else changed: a peak key or a ramp offset made for D ** -0.5 keeps its
K values, so its score moves with the scale (a peak of 16 becomes 38 at D = 64 and fp32(0.3), a ramp of 1e4 becomes 2.4e4).

Scales.  SCALES(D) = 1.0, fp32(0.3), fp32(fp32(1/3) fp32(D ** -0.5)), 2^-20, 4.0: two that are no power of two (a scale applied anywhere
but as the one fp32 product t_j = a_j * softmax_scale rounds differently there - at a power of two it does not), a tiny and a large one.
2^-149, the smallest positive subnormal fp32, is the least scale the entry points accept ("finite and positive"): every score is then
zero or subnormal and the witness's weights are uniform to 1e-40.  Scales at which a score OVERFLOWS fp32 (|a_j| softmax_scale >= 2^128)
are outside the header's "finite inputs" and are not tested: the contract says nothing about them.

Value kinds on unequal lengths (the recipes are tests/_attn_cases.py's, on `_attn_var_cases.build`'s Gaussian tensors):
  vmax     v = +-65504 (fp16) / +-2^100 (bf16)
  zeroq    q = 0: every score 0 whatever the scale - only the key COUNT decides lse = log K, bit for bit the same at every scale
  equal    q = 0.5, every key 0.25: all scores equal and non-zero
  int      q, k integers in -3 .. 3: a score's fp32 sum a is exact; sks = [1]: out is v's bits and lse is fp32(a * scale) bit for bit

Query counts.  SQS = 31 .. 257 around 32, 64, 128, 256 - where nqt = ceil(Sq / qtile) and wave_on = q0 < Sq sit on their boundary for the
three query tiles.  Every Sq case of one (entry point, D) is the q PREFIX of ONE Sq = 257 case over the same blocks (B = 1: the prefix is
contiguous), so that a row can be compared bit for bit between launches.

MOVED lists the cases that sit on a neighbouring shape because the one the list calls for does not exist for their entry point.
"""
import zlib

import numpy as np

import _attn_cases as C
import _attn_var_cases as VC

ENTRIES = ("eq", "var", "hd")
DIMS = {"eq": (64, 128), "var": (64, 128), "hd": (72, 88, 120)}
INT_DIMS = {"var": (64, 128), "hd": (72, 80, 88, 96, 104, 112, 120)}
HEADS = {"eq": 2, "var": 2, "hd": 3}
SCALE_NAMES = ("one", "p3", "third", "tiny", "four")
LISTS = ([65, 64, 63], [100, 37, 128, 5])
EQ_SHAPES = ((65, 3), (100, 2))                             # (Sk, n) of the equal launch's scale cases
KIND_LISTS = ([65, 64, 63], [100, 37, 128, 5], list(range(1, 17)))
FLAT_KINDS = ("vmax", "zeroq", "equal")
SQS = (31, 32, 63, 64, 65, 127, 128, 255, 256, 257)
SQ_TOP = 257
SQ_DIMS = (("eq", 64), ("var", 64), ("hd", 72), ("hd", 120))
SQ_BF16 = (128, 256)
SUBNORMAL = float(np.float32(2.0 ** -149))

# (the case the list calls for, what runs instead, why)
MOVED = (
    ("sq: eq on [65, 64, 63]", "sq: eq on Sk 65, n 3", "cfx_attn_fwd_blocks takes blocks of ONE length: three blocks of 65 keys keep the tail tile in every block"),
)


def scale_of(sname, D):
    """the named scale as a Python float that is an fp32 value"""
    f = np.float32
    return float({"one": f(1.0), "p3": f(0.3), "third": f(f(1.0 / 3.0) * f(D ** -0.5)), "tiny": f(2.0 ** -20), "four": f(4.0),
                  "def": f(D ** -0.5), "sub": f(2.0 ** -149)}[sname])


def _shape_tag(c):
    return f"k{c['Sk']}-n{c['n']}" if c["ep"] == "eq" else VC._tag(c["sks"])


def _cases():
    out = []

    def add(ep, group, kind, D, sname, Sq=33, B=2, sks=None, Sk=None, n=None, dtypes=("fp16", "bf16"), **kw):
        c = dict(ep=ep, group=group, kind=kind, D=D, H=HEADS[ep], B=B, Sq=Sq, sname=sname, scale=scale_of(sname, D), dtypes=tuple(dtypes), **kw)
        if ep == "eq":
            c.update(Sk=Sk, n=n)
        else:
            c.update(sks=list(sks))
        tag = "".join(f"-{k}{v}" for k, v in kw.items())
        c["id"] = f"{ep}-{group}-{kind}{tag}-{sname}-q{Sq}-{_shape_tag(c)}-b{B}-d{D}"
        out.append(c)
    # ---- scales: every scale x entry point x D x two shapes, gaussian; peak and ramp once per entry point at fp32(0.3); 2^-149 once
    for ep in ENTRIES:
        for D in DIMS[ep]:
            for i in range(2):
                shape = dict(Sk=EQ_SHAPES[i][0], n=EQ_SHAPES[i][1]) if ep == "eq" else dict(sks=LISTS[i])
                for sname in SCALE_NAMES:
                    add(ep, "scale", "gauss", D, sname, **shape)
        D = DIMS[ep][0]
        if ep == "eq":
            add(ep, "scale", "peak", D, "p3", Sk=65, n=3, where="tail")
            add(ep, "scale", "ramp", D, "p3", Sk=65, n=3)
            add(ep, "scale", "gauss", D, "sub", Sk=100, n=2)
        else:
            add(ep, "scale", "peak", D, "p3", sks=LISTS[1], pblk=1, pend="last")
            add(ep, "scale", "ramp", D, "p3", sks=LISTS[0])
            add(ep, "scale", "gauss", D, "sub", sks=LISTS[1])
    # ---- the flat value kinds on unequal lengths, at the default scale
    for ep in ("var", "hd"):
        for D in DIMS[ep]:
            for sks in KIND_LISTS:
                for kind in FLAT_KINDS:
                    add(ep, "kind", kind, D, "def", sks=sks)
    # ---- the single key held bit for bit, at every D, at D ** -0.5 and at fp32(0.3); three blocks of one key once per entry point
    for ep in ("var", "hd"):
        for D in INT_DIMS[ep]:
            for sname in ("def", "p3"):
                add(ep, "int", "int", D, sname, sks=[1])
        add(ep, "int", "int", INT_DIMS[ep][0], "p3", sks=[1, 1, 1])
    # ---- query counts: B = 1, fp16; bf16 at two whole-tile counts (and at the 257 rows the others are prefixes of)
    for ep, D in SQ_DIMS:
        for Sq in SQS:
            dt = ("fp16", "bf16") if Sq in SQ_BF16 + (SQ_TOP,) else ("fp16",)
            shape = dict(Sk=65, n=3) if ep == "eq" else dict(sks=LISTS[0])
            add(ep, "sq", "gauss", D, "def", Sq=Sq, B=1, dtypes=dt, **shape)
    return out


CASES = _cases()


def of(ep=None, group=None, dtype=None, **eq):
    """the cases of an entry point / group / element type whose fields equal `eq`"""
    return [c for c in CASES if (ep is None or c["ep"] == ep) and (group is None or c["group"] == group)
            and (dtype is None or dtype in c["dtypes"]) and all(c.get(k) == v for k, v in eq.items())]


def lengths(case):
    """the blocks' key counts"""
    return [case["Sk"]] * case["n"] if case["ep"] == "eq" else list(case["sks"])


def sq_base(case):
    """the Sq = 257 case an `sq` case is a prefix of (the same dict for every Sq of one entry point and D)"""
    assert case["group"] == "sq"
    return next(c for c in CASES if c["group"] == "sq" and c["ep"] == case["ep"] and c["D"] == case["D"] and c["Sq"] == SQ_TOP)


def _gauss_like(case):
    """the case as the existing builders know it: their Gaussian tensors under the kinds they do not have"""
    return dict(case, kind="gauss") if case["kind"] in FLAT_KINDS + ("int",) and case["ep"] != "eq" else case


def build(case, dtype):
    """(q, ks, vs, scale): the existing builder's tensors, the value kinds of _attn_cases on unequal lengths, the case's own scale"""
    assert dtype in case["dtypes"], (case["id"], dtype)
    if case["group"] == "sq" and case["Sq"] != SQ_TOP:
        q, ks, vs, scale = build(sq_base(case), dtype)
        return np.ascontiguousarray(q[:, :case["Sq"]]), ks, vs, scale
    if case["ep"] == "eq":
        q, ks, vs, _ = C.build(case, dtype)
        return q, ks, vs, case["scale"]
    q, ks, vs, _ = VC.build(_gauss_like(case), dtype)
    kind = case["kind"]
    rng = np.random.default_rng(zlib.crc32((case["id"] + dtype + "/kind").encode()))
    if kind == "vmax":
        top = 65504.0 if dtype == "fp16" else 2.0 ** 100
        vs = [C.to_elem(np.where(rng.random(v.shape) < 0.5, -top, top), dtype) for v in vs]
    elif kind == "zeroq":
        q = np.zeros_like(q)
    elif kind == "equal":
        q = np.full_like(q, 0.5)
        ks = [np.full_like(k, 0.25) for k in ks]
    elif kind == "int":
        q = C.to_elem(rng.integers(-3, 4, q.shape), dtype)
        ks = [C.to_elem(rng.integers(-3, 4, k.shape), dtype) for k in ks]
    return q, ks, vs, case["scale"]
