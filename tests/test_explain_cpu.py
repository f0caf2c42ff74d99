"""CPU side of the explain feature (`pmx_explain`), pinned to the reference's own tree search: tests/golden/explain_<set>.npz hold, per
chosen ligand, the reference's per-conformer maxima, levels, the key of the first leaf that reaches each maximum and the gap to the
best leaf with another key (tests/golden/make_golden_explain.py). The NumPy restatement of tests/explain_ref.py - a leaf's total
`path_score`, the tree walked in iteration order with the tie rule - must reproduce them; the GPU tests (test_gpu_explain.py) use the
same helpers where no fixture exists."""

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from explain_ref import NONE, Tables, first_max_key, ligand_levels, path_score, tree_leaves

EXPLAIN_SETS = ("set_6oim_c8", "set_6oim_c1", "set_6oim_c64", "set_c21_c8", "set_6oim_c8_weights", "set_s64_c8")


def load_explain(name):
    """(model, library, weights, set npz, explain fixture) of a golden set."""
    model, lib, weights, d = load_golden(name)
    return model, lib, weights, d, np.load(GOLDEN / f"explain_{name}.npz")


def fixture_rows(x):
    """Per fixture ligand: (library index, C, levels [nl], scores [C], keys [C, nl] with -1 for None, gaps [C])."""
    for r, i in enumerate(x["index"]):
        C = int(x["n_conf"][r])
        lv = x["levels"][r]
        nl = int(np.count_nonzero(lv != 0xFE))
        key = x["key"][r, :C, :nl].astype(np.int64)
        key[key == 0xFF] = NONE
        yield int(i), C, lv[:nl].astype(np.int64), x["scores"][r, :C], key, x["gap"][r, :C]


@pytest.mark.parametrize("name", EXPLAIN_SETS)
def test_path_score_of_the_reference_key_is_the_reference_maximum(name):
    from pharmaconet_amd.constants import weights_vector

    model, lib, weights, _, x = load_explain(name)
    w7 = weights_vector(weights)
    n = 0
    for i, C, lv, sc, key, _ in fixture_rows(x):
        rec = lib.unpack(i)
        T = Tables(model, rec, w7)
        assert ligand_levels(model, rec) == lv.tolist()
        for c in range(C):
            if sc[c] > 0:
                assert abs(path_score(model, rec, w7, lv, key[c], c, T) - sc[c]) <= 2e-6 * sc[c], (name, i, c)
                n += 1
            else:
                assert (key[c] == NONE).all()
    assert n > 0


@pytest.mark.parametrize("name", EXPLAIN_SETS)
def test_key_rule_reproduces_the_reference_keys(name):
    """The restated tree's leaves, with the rule as written (first leaf in iteration order at the maximum), give the reference's key
    wherever the runner-up with another key is more than 1e-5 below; within that gap, a key whose total is the maximum."""
    from pharmaconet_amd.constants import weights_vector

    model, lib, weights, d, x = load_explain(name)
    w7 = weights_vector(weights)
    exact = 0
    for i, C, lv, sc, key, gap in fixture_rows(x):
        if d["n_tree"][i] > 3000:
            continue
        rec = lib.unpack(i)
        T = Tables(model, rec, w7)
        levels, leaves = tree_leaves(model, rec, w7, T)
        assert levels == lv.tolist() and len(leaves) == int(d["n_leaf"][i])
        best, keys = first_max_key(leaves, C)
        assert np.allclose(best, sc, rtol=2e-6, atol=0), (name, i)
        for c in range(C):
            if sc[c] <= 0:
                assert keys[c] is None
            elif gap[c] > 1e-5:
                assert keys[c] == tuple(key[c].tolist()), (name, i, c)
                exact += 1
            else:
                assert abs(path_score(model, rec, w7, lv, keys[c], c, T) - sc[c]) <= 2e-6 * sc[c]
    assert exact > 0


def test_key_rule_on_a_made_up_tie():
    leaves = [([0, NONE], {0: 1.0, 1: 2.0}), ([1, 2], {0: 3.0}), ([1, NONE], {0: 3.0, 1: 2.0}), ([NONE, 2], {1: 5.0})]
    best, keys = first_max_key(leaves, 3)
    assert best.tolist() == [3.0, 5.0, 0.0]
    assert keys == [(1, 2), (NONE, 2), None]
