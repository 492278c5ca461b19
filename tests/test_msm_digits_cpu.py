"""CPU tests of tests/msm_digits_util.py: the Python restatement of the MSM's signed-digit recoding holds on every special scalar, the
special scalars really contain the edges the GPU test (tests/test_gpu_msm_edges.py) is there for, and the model's window count is the
library's (mi_test_plan, host only).  These are conditions on the test INPUTS, not measurements of the kernels."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msm_digits_util as du  # noqa: E402


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("c", du.C_ALL)
def test_recoding_model_on_the_special_scalars(o, c, fold):
    r = o.R_ORDER
    vals = du.special_scalars(c, r)
    assert all(0 <= v < (1 << 256) for v in vals)
    for want in (0, 1, 2, r - 2, r - 1, r, r + 1, 2 * r, 2 * r + 1, (r - 1) // 2 - 1, (r - 1) // 2, (r + 1) // 2, (r + 1) // 2 + 1,
                 (1 << 255) - 1, (1 << 256) - 1):
        assert want in vals
    seen = set()
    half = 1 << (c - 1)
    for v in vals:
        d, ev = du.recode(v, c, fold, r)            # asserts: no carry out of the last window, the digits sum back to v mod r
        assert len(d) == du.windows(c, fold)
        assert all(-half <= x <= half for x in d)
        seen |= ev
    assert {du.TIE, du.FIRST_NEG, du.ZERO_CARRY, du.TOP_NONZERO} <= seen
    assert (du.FLIPPED in seen) == fold
    if not fold and c in (15, 17):
        assert du.TOP_CARRY_ONLY in seen
    # the fold threshold itself: (r - 1) / 2 stays, (r + 1) / 2 flips to (r - 1) / 2 with every sign inverted
    lo, _ = du.recode((r - 1) // 2, c, fold, r)
    hi, ev = du.recode((r + 1) // 2, c, fold, r)
    if fold:
        assert du.FLIPPED in ev and hi == [-x for x in lo]
    else:
        assert sum(x << (c * j) for j, x in enumerate(hi)) == (r + 1) // 2


def test_a_whole_vector_of_ties_and_a_carry_through_every_window(o):
    """what the constructed patterns are for, spelled out at one window size"""
    r, c = o.R_ORDER, 8
    n = 253 // c
    d, ev = du.recode(du._pattern(c, 128, 128, 253), c, False, r)
    assert d[:n] == [128] * n and ev >= {du.TIE}
    d, ev = du.recode(du._pattern(c, 129, 255, 253), c, False, r)
    assert d[:n + 1] == [-127] + [0] * (n - 1) + [1] and du.ZERO_CARRY in ev
    d, ev = du.recode(du._pattern(c, 129, 129, 253), c, False, r)
    assert d[:n + 1] == [-127] + [-126] * (n - 1) + [1]
    d, ev = du.recode(r - du._pattern(c, 128, 128, 253), c, True, r)
    assert d[:n] == [-128] * n and du.FLIPPED in ev


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_window_count_is_the_plans(pkg, group):
    for c in du.C_ALL:
        for fold in (False, True):
            for n in (300, 5000):
                p = pkg.test_plan(n, c, group, False, 0, fold)
                assert p["c"] == c and p["nwin"] == du.windows(c, fold), (c, fold, n)
