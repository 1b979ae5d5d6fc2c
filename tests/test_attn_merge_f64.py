"""The block merge's float64 reference and derived bound (tests/_merge_f64.py) on the CPU: the eager fp32 formula and a numpy fp32
transcription of attn_merge_body (its exponential moved by the stated error of __expf, both ways) meet the bound over the case list
tests/test_gpu_attn_merge_f64.py holds the kernels to; the bound is not vacuous; the check rejects planted errors.  CPU only."""
import numpy as np
import pytest

import _merge_f64 as M

SMALL = [c for c in M.CASES if c["shape"] != M.FLUX]


@pytest.mark.parametrize("case", M.CASES, ids=[c["id"] for c in M.CASES])
def test_fp32_forms_meet_the_bound(case):
    blocks = M.build(case)
    o, l = M.eager_fp32(blocks)
    fo, fl = M.check(o, l, blocks, "eager fp32 formula")
    print(f"{case['id']}: eager {fo:.3f} / {fl:.3f} of the bound (out / lse)")
    for err in (0.0, 1.0, -1.0):
        if err and case["shape"] == M.FLUX:
            continue
        o, l = M.kernel_fp32(blocks, exp_err=err)
        ko, kl = M.check(o, l, blocks, f"attn_merge_body in numpy fp32, exponential off by {err:+.0f} x its stated error")
        print(f"{case['id']}: transcription ({err:+.0f}) {ko:.3f} / {kl:.3f}")


def test_case_list_covers_what_it_claims():
    cs = M.CASES
    assert {c["shape"][3] for c in cs} >= set(M.HEAD_DIMS)
    for D in M.HEAD_DIMS:
        lg = 0
        while (1 << lg) < D // 8:
            lg += 1
        rows = [c["shape"][0] * c["shape"][1] * c["shape"][2] for c in cs if c["shape"][3] == D]
        assert any((r << lg) % 256 for r in rows) and any((r << lg) % 256 == 0 for r in rows), D
    assert any(c["shape"][1] == 1 for c in cs) and any(c["shape"][2] == 1 for c in cs) and any(c["shape"][0] == 1 for c in cs)
    assert any(c["shape"] == M.FLUX for c in cs)
    assert {c["n"] for c in cs} == {2, 4, 15}
    for dtype in ("fp16", "bf16"):
        mine = [c for c in cs if c["dtype"] == dtype]
        assert {c["gap"] for c in mine} == set(M.GAPS)
        assert {c["offset"] for c in mine} == {0.0, 300.0, -300.0}
        assert {c["gap"] for c in mine if c["mag"] == "max"} == set(M.GAPS)
    b = M.build(next(c for c in cs if c["dtype"] == "fp16" and c["mag"] == "max"))
    assert max(np.abs(o).max() for o, _ in b) == 65504.0
    b = M.build(next(c for c in cs if c["dtype"] == "bf16" and c["mag"] == "max"))
    assert max(np.abs(o).max() for o, _ in b) == 2.0 ** 100
    # the gaps the chains really have (fp32 lse): each class reaches its nominal size
    for gap, want in (("zero", 0.0), ("unit", 1.0), ("mid", 20.0), ("far", 90.0), ("huge", 1e4)):
        c = next(c for c in cs if c["gap"] == gap and c["offset"] == 0.0 and c["mag"] == "unit")
        blocks = M.build(c)
        x = blocks[-1][1].astype(np.float64) - M.reference_and_bound(blocks[:-1])[1]
        assert abs(np.abs(x).max() - want) <= 1e-3 * max(want, 1e-3) and (x.min() < 0 or want == 0) and x.max() >= 0, (gap, x.min(), x.max())


@pytest.mark.parametrize("gap", list(M.GAPS))
def test_the_bound_is_not_vacuous(gap):
    """on at least one case of every gap class the eager formula's worst error reaches an eighth of the bound"""
    best = 0.0
    for c in SMALL:
        if c["gap"] != gap:
            continue
        blocks = M.build(c)
        fo, fl = M.check(*M.eager_fp32(blocks), blocks)
        best = max(best, fo)
    print(f"gap class {gap}: the eager formula reaches {best:.3f} of the bound")
    assert best >= 0.125, best


# ---- planted errors -------------------------------------------------------------------------------------------------------------------
# (at a unit gap every one of these moves the result by a tenth of its size or more; at |gap| >= 20 the sigmoid is 0 or 1 to fp32 and a
# row merged with a stale or a foreign lse can be the right answer)
PLANT = [c for c in SMALL if c["gap"] == "unit"]


@pytest.mark.parametrize("case", PLANT, ids=[c["id"] for c in PLANT])
def test_the_check_rejects_planted_errors(case):
    blocks = M.build(case)
    B, S, H, D = case["shape"]
    M.check(*M.kernel_fp32(blocks), blocks)
    last = len(blocks) - 1
    row = (B - 1, S // 2, H - 1)

    def updated_lse(body, o, l, ob, lb, k):
        """one row merged with the lse its own launch has already rewritten (what a row spread over two waves could read)"""
        o2, l2 = body(o, l, ob, lb)
        if k == last:
            o3, _ = body(o, l2, ob, lb)
            o2[row] = o3[row]
        return o2, l2

    def neighbour_lse(body, o, l, ob, lb, k):
        o2, l2 = body(o, l, ob, lb)
        if k == last:
            o3, _ = body(o, np.roll(l.reshape(-1), 1).reshape(l.shape), ob, lb)
            o2[row] = o3[row]
        return o2, l2

    def no_lse_update(body, o, l, ob, lb, k):
        o2, l2 = body(o, l, ob, lb)
        if k == last:
            l2[row] = l[row]
        return o2, l2

    def lane_unmerged(body, o, l, ob, lb, k):
        o2, l2 = body(o, l, ob, lb)
        if k == last:
            o2[row][D - 8:] = o[row][D - 8:]
        return o2, l2
    for plant, where in ((updated_lse, "out"), (neighbour_lse, "out"), (no_lse_update, "lse"), (lane_unmerged, "out")):
        with pytest.raises(AssertionError, match=f"{where}: 1?[0-9]*/"):
            M.check(*M.kernel_fp32(blocks, merge=plant), blocks, plant.__name__)
