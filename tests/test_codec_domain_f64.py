"""The numpy oracle against the float64 definition of every codec (tests/_f64_check.py) over the shape domain the C-ABI accepts
(tests/_domain_cases.py): pins the oracle on the shapes the GPU sweep (tests/test_gpu_codec_domain.py) holds the kernels to.  CPU only."""
import numpy as np
import pytest

import _domain_cases as D
import _f64_check as F
from oracle import ref_np as R


def inputs(seed, N, C):
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((N, C)).astype(np.float16)
    x = (base.astype(np.float32) + 0.1 * rng.standard_normal((N, C)).astype(np.float32)).astype(np.float16)
    return x, base


def _cases():
    out = []
    for (name, _, param), cid in zip(D.CODECS, D.CODEC_IDS):
        for N, C in D.shapes_for(name, param):
            out.append(pytest.param(name, param, N, C, id=f"{cid}-{N}x{C}"))
    return out


@pytest.mark.parametrize("name,param,N,C", _cases())
def test_oracle_meets_f64_definition(name, param, N, C):
    x, base = inputs(N * 131 + C, N, C)
    pkt, nb = R.residual_compress(name, x, base, param)
    F.check(name, param, x, base, pkt, R.bits(nb))
    pkt0, recv0 = R.compress(name, x, None, param)                  # residual 0: d = x
    F.check(name, param, x, None, pkt0, R.bits(recv0))


@pytest.mark.parametrize("name,param", [(n, p) for n, _, p in D.CODECS])
def test_domain_has_every_case_kind(name, param):
    """the case list itself: enough legal shapes, odd N (where legal), C % 16 == 8, CB = 46 and 47, and a packet whose tail sections are
    not 16-byte aligned - except top-k, whose index section starts at 2*N*C/m bytes, a multiple of 128 for every legal shape"""
    shapes = D.shapes_for(name, param)
    assert len(shapes) >= (8 if name == "topk" else 14), shapes
    assert any(C % 16 == 8 for _, C in shapes)
    assert any((C + 511) // 512 == D.TICK_MAX_CB for _, C in shapes)
    assert any((C + 511) // 512 == D.TICK_MAX_CB + 1 for _, C in shapes)
    if name != "int4":
        assert any(N % 2 for N, _ in shapes)
    if name == "topk":
        assert all(D.tails_aligned(name, N, C, param) for N, C in shapes)
        assert any(C % 1024 and (1024 % C or C > 1024) for _, C in shapes)        # flat blocks straddle rows
    else:
        un = [(N, C) for N, C in shapes if not D.tails_aligned(name, N, C, param)]
        assert un, f"{name}: no shape with an unaligned tail section"
    for pool in (D.FINALIZE_OFF, D.BATCH_SHAPES, D.GATED_SHAPES, D.GRAPH_SHAPES):
        assert D.subset(name, param, pool), (name, param)
    if name in ("int8", "int4"):
        for pool in (D.FINALIZE_OFF, D.GATED_SHAPES):
            assert any(not D.tails_aligned(name, N, C) for N, C in D.subset(name, param, pool)), pool
