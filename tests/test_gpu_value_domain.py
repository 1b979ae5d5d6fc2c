"""The int8, int4 and top-k kernels over their VALUE domain (tests/_value_cases.py) in every launch form (GPU box only, -m gpu): every case at
the smallest shape that takes the form - which the test proves by the kernel ids the call launched - through (a) the plain compress +
decompress (the stand-alone dequantisers), with a base over two rounds of error feedback (the second round's residual is the first round's
quantisation error) and with base None, and (b) the gated layer call with looped-back peers (the layer launch's D tiles where the form has
them) over two rounds.  Every run: packets against the numpy oracle (int4's `min` half under the signed-zero rule, tests/_zero_min.py, used
on planted channels only), sender state, receiver reconstruction and peer states bit for bit, the float64 definition (tests/_f64_check.py)
wherever the case is finite, no gate error.

Forms (read from cfx_i_minmax_compress / cfx_i_topk_compress; MM_FORMS / TK_FORMS below):
  layer launch (kernel id 31 alone; C % 16 == 0): S tiles of 32 rows (N <= 1024) or 64, every tile reducing its column block's partials
  itself; the cooperative reduce (more than 32 partials a channel); the tall form (more than 64); k_minmax_compress (29; C % 16 == 8), the
  quantiser (9 / 11) and, gated, the dequantiser (10 / 12) behind it; k_minmax_stats + k_minmax_finalize (7, 8; in-launch finalize off) at rows
  per tile 0 / 16 / 128; one and two rows; top-k: k_topk_compress / k_topk_decompress (13, 14) and k_topk_layer (31)."""
import numpy as np
import pytest
import torch

import _f64_check as F
import _value_cases as V
from _gpu_codec import KID_LAYER, _gated_layer, _profile, dev, host, oracle, same_bits, same_packet

pytestmark = pytest.mark.gpu

F16 = np.float16
CID = {"int4": 3, "int8": 4, "topk": 5}
QUANT, DEQUANT = {"int8": 9, "int4": 11}, {"int8": 10, "int4": 12}
KID_STATS, KID_FINALIZE, KID_MM_COMPRESS, KID_TK_COMPRESS, KID_TK_DECOMPRESS = 7, 8, 29, 13, 14

# (form, shapes, in-launch finalize, rows per tile, the layer launch's sub-form or None)
MM_FORMS = [
    ("layer-32-row-tiles", [(66, 144), (66, 528)], True, 0, "S32"),
    ("layer-64-row-tiles", [(1026, 16)], True, 0, "S64"),
    ("layer-cooperative-reduce", [(2050, 16)], True, 0, "coop"),
    ("layer-tall", [(4098, 16)], True, 0, "tall"),
    ("minmax-compress", [(66, 136), (18, 24)], True, 0, None),
    ("stats-finalize-rows-0", [(66, 136), (66, 144)], False, 0, None),
    ("stats-finalize-rows-16", [(66, 136), (66, 144)], False, 16, None),
    ("stats-finalize-rows-128", [(66, 136), (66, 144)], False, 128, None),
    ("one-and-two-rows", [(1, 72), (2, 72)], True, 0, None),
]
TK_FORMS = [("plain-and-layer", V.TOPK_SHAPES)]


def layer_sub_form(N):
    """cfx_i_minmax_compress: RL, PL, coop, tall (MML_MAX_P = 64)"""
    RL = 32 if (N + 31) // 32 <= 32 else 64
    PL = (N + RL - 1) // RL
    return "tall" if PL > 64 else ("coop" if PL > 32 else f"S{RL}")


def want_ids(codec, form):
    """(plain compress, plain decompress, gated call) kernel ids of a form"""
    if codec == "topk":
        return [KID_TK_COMPRESS], [KID_TK_DECOMPRESS], [KID_LAYER]
    q, dq = QUANT[codec], DEQUANT[codec]
    if form.startswith("layer"):
        return [KID_LAYER], [dq], [KID_LAYER]
    if form.startswith("stats-finalize"):
        return [KID_STATS, KID_FINALIZE, q], [dq], [KID_STATS, KID_FINALIZE, q, dq]
    return [KID_MM_COMPRESS, q], [dq], [KID_MM_COMPRESS, q, dq]


@pytest.fixture(autouse=True)
def _defaults():
    from compactfusion_amd import codecs as K
    yield
    K.set_fused_finalize(True)
    K.set_rows_per_tile(0)


def _plain(codec, param, x, base, rounds, finite, allowed, what):
    """compress + decompress over `rounds` rounds of error feedback; returns the kernel ids of the first compress and decompress"""
    from compactfusion_amd import _lib, codecs as K
    lib, ctx, cid = _lib.load(), K.context(0), CID[codec]
    N, C = x.shape
    xd = dev(x)
    bd = None if base is None else dev(base)
    state, ids = base, None
    for t in range(rounds):
        pkt_ref, nb_ref = oracle(codec, x, state, param, N, C)
        out = {}

        def comp():
            out["pkt"], out["nb"] = K.compress(cid, xd, bd, N, C, param, update_cache=True)

        def dec():
            out["rec"] = K.decompress(cid, out["pkt"], bd, N, C, param)
        if ids is None:
            ids = (_profile(ctx, lib, comp), _profile(ctx, lib, dec))
        else:
            comp()
            dec()
        torch.cuda.synchronize()
        hp, hn = host(out["pkt"]), host(out["nb"]).reshape(N, C)
        same_packet(codec, hp, pkt_ref, x, state, f"{what}: packet round {t}", allowed)
        same_bits(hn, nb_ref, f"{what}: sender state round {t}")
        same_bits(host(out["rec"]), nb_ref, f"{what}: receiver reconstruction round {t}")
        if finite:
            F.check(codec, param, x, state, hp, hn)
        bd, state = out["nb"], nb_ref.view(F16).reshape(N, C)
    assert lib.cfx_gate_errors(ctx) == 0
    return ids


def _run(codec, param, form, N, C, case):
    want_c, want_d, want_g = want_ids(codec, form)
    finite = case in V.FINITE
    allowed = set()
    for rep in range(V.reps(case, N, C)):
        x, base = V.build(case, codec, N, C, rep=rep, param=param)
        ids = _plain(codec, param, x, base, 2 if rep == 0 else 1, finite, allowed, f"{case} rep {rep}")
        assert ids == (want_c, want_d), (form, N, C, ids)
    x0, _ = V.build(case, codec, N, C, param=param, nobase=True)
    ids = _plain(codec, param, x0, None, 1, finite, allowed, f"{case} base None")
    assert ids == (want_c, want_d), (form, N, C, ids)
    ins = [V.build(case, codec, N, C, rep=r, param=param) for r in (0, 1)]
    ids = _gated_layer(codec, CID[codec], param, N, C, B=2, NP=3, rounds=2, seed=0, ins=ins, allowed=allowed, f64=finite)
    assert ids == want_g, (form, N, C, ids)
    assert allowed <= V.signed_zero_channels(case, N, C), f"the signed-zero rule was used on channels {sorted(allowed)} that the case does not plant"


def _mm_params():
    out = []
    for codec in V.MINMAX:
        for form, shapes, fused, rows, sub in MM_FORMS:
            for N, C in shapes:
                if not V.legal(codec, N, C):
                    continue
                for case in V.cases_for(codec, N, C):
                    out.append(pytest.param(codec, form, fused, rows, sub, N, C, case, id=f"{codec}-{form}-{N}x{C}-{case}"))
    return out


@pytest.mark.parametrize("codec,form,fused,rows,sub,N,C,case", _mm_params())
def test_minmax_value_domain(codec, form, fused, rows, sub, N, C, case):
    from compactfusion_amd import codecs as K
    assert sub is None or layer_sub_form(N) == sub
    K.set_fused_finalize(fused)
    K.set_rows_per_tile(rows)
    _run(codec, 0, form, N, C, case)


def _tk_params():
    return [pytest.param(m, N, C, case, id=f"topk{m}-{N}x{C}-{case}")
            for m in V.TOPK_M for form, shapes in TK_FORMS for N, C in shapes for case in V.cases_for("topk", N, C, m)]


@pytest.mark.parametrize("m,N,C,case", _tk_params())
def test_topk_value_domain(m, N, C, case):
    _run("topk", m, "plain-and-layer", N, C, case)


# ---- coverage: every form of the table ran, for every codec ----
def test_coverage_every_form_for_every_codec():
    """one case through every form and shape of the tables, by itself: the kernel ids of the plain compress, the plain decompress and the gated
    call are the form's, and the layer launch's shapes fall on the sub-form the table names.  A changed dispatch rule fails here (and in the
    tests above) instead of moving the cases to another form unnoticed."""
    from compactfusion_amd import _lib, codecs as K
    lib, ctx = _lib.load(), K.context(0)
    seen = {}
    for codec in V.MINMAX:
        for form, shapes, fused, rows, sub in MM_FORMS:
            K.set_fused_finalize(fused)
            K.set_rows_per_tile(rows)
            for N, C in shapes:
                if not V.legal(codec, N, C):
                    continue
                assert (sub is None) == (C % 16 != 0 or not fused) and (sub is None or layer_sub_form(N) == sub), (form, N, C)
                x, base = V.build("tiny", codec, N, C)
                out = {}
                ic = _profile(ctx, lib, lambda: out.update(p=K.compress(CID[codec], dev(x), dev(base), N, C, 0, update_cache=True)))
                idd = _profile(ctx, lib, lambda: K.decompress(CID[codec], out["p"][0], dev(base), N, C, 0))
                ig = _gated_layer(codec, CID[codec], 0, N, C, B=2, NP=3, rounds=1, seed=0, check=False, ins=[(x, base), (x, base)])
                assert (ic, idd, ig) == want_ids(codec, form), (codec, form, N, C, ic, idd, ig)
                seen.setdefault(codec, set()).add(form)
    K.set_fused_finalize(True)
    K.set_rows_per_tile(0)
    for m in V.TOPK_M:
        for N, C in V.TOPK_SHAPES:
            x, base = V.build("ties", "topk", N, C, param=m)
            out = {}
            ic = _profile(ctx, lib, lambda: out.update(p=K.compress(5, dev(x), dev(base), N, C, m, update_cache=True)))
            idd = _profile(ctx, lib, lambda: K.decompress(5, out["p"][0], dev(base), N, C, m))
            ig = _gated_layer("topk", 5, m, N, C, B=2, NP=3, rounds=1, seed=0, check=False, ins=[(x, base), (x, base)])
            assert (ic, idd, ig) == want_ids("topk", "plain-and-layer"), (m, N, C, ic, idd, ig)
            seen.setdefault(f"topk{m}", set()).add((N, C))
    assert lib.cfx_gate_errors(ctx) == 0
    forms = {f for f, *_ in MM_FORMS}
    assert seen["int4"] == forms and seen["int8"] == forms, (forms - seen["int4"], forms - seen["int8"])
    for m in V.TOPK_M:
        assert seen[f"topk{m}"] == set(V.TOPK_SHAPES)
    assert {s for _, _, _, _, s in MM_FORMS if s} == {"S32", "S64", "coop", "tall"}
