"""What keeps the lane-shape tests of the tail arms honest, from the oracle alone (no GPU): the libraries of tests/tail_cases.py and of
test_gpu_explain_shapes.py's spread-weight cases reach what tests/test_gpu_tail_shapes.py and tests/test_gpu_explain_shapes.py assert on."""

import numpy as np
import pytest

from tail_cases import FLOOR, PAIR_SHAPE_SETS, SELF_SHAPES, SHAPES, WEIGHT_SETS, pair_shape_cases, pair_shape_explained, self_shape_cases
from test_gpu_explain_shapes import SPREAD_CONFORMERS, SPREAD_LIBRARIES, SPREAD_WEIGHTS, honest, sweep_cases


@pytest.mark.parametrize("wname,sigma_min_to", PAIR_SHAPE_SETS)
def test_pair_shape_libraries_are_mostly_tail_where_it_counts(wname, sigma_min_to):
    """Six cluster pairs per shape, every record with a valid pair entry, and at least a tenth of a shape's records mostly the one tail item."""
    for C in SHAPES:
        cases = pair_shape_cases(wname, sigma_min_to, C)
        assert len(cases) == 6, C
        n, n_tail = 0, 0
        for c in cases:
            assert len(c.lib) == -(-1600 // C) and all(c.lib.header(i)[1] == C for i in (0, len(c.lib) - 1))
            assert c.valid.all() and (c.ref > FLOOR).all(), (C, c.a, c.b)
            n += len(c.ref)
            n_tail += int(c.mostly_tail.sum())
        print(f"[{wname}] C={C}: {n_tail} of {n} records mostly one tail item ({100 * n_tail / n:.1f} %)")
        assert 10 * n_tail >= n, (C, n_tail, n)


def test_pair_shape_explanations_are_the_scores_walk():
    """The oracle's explanation of those libraries: every conformer has a best leaf, and the mean of the maxima is its score."""
    wname, sigma_min_to = PAIR_SHAPE_SETS[0]
    for C in SHAPES:
        for c, ref in zip(pair_shape_cases(wname, sigma_min_to, C), pair_shape_explained(wname, sigma_min_to, C)):
            assert (ref["values"][:, 0, :C] > 0).all() and (ref["values"][:, :, C:] == 0).all()
            assert np.array_equal(ref["scores"], c.ref)


def test_self_shape_libraries_reach_the_tails():
    """Three clusters per shape; each sweep runs from scores above the floor to scores below it, so it crosses the tails on the way."""
    for C in SELF_SHAPES:
        cases = self_shape_cases(C)
        assert len(cases) == 3 and len({c.a for c in cases}) == 3
        for c in cases:
            assert c.lib.header(0)[1] == C
            sel = c.ref > FLOOR
            assert sel.any() and (~sel).any(), (C, c.a)


@pytest.mark.parametrize("wname", SPREAD_WEIGHTS)
@pytest.mark.parametrize("conformers", SPREAD_CONFORMERS)
def test_spread_weight_libraries_are_honest(conformers, wname):
    """`honest()` as test_explain_family_under_spread_weights asserts it: more than half of each library scores, at least half of the entries
    are compared by key."""
    top, exact = honest(sweep_cases(conformers, WEIGHT_SETS[wname], SPREAD_LIBRARIES))
    print(f"C={conformers} [{wname}]: key-exact share of the oracle's entries: maxima {top:.3f}, modes {exact:.3f}")
