"""CPU side of binding modes (`pmx_explain_modes`): tests/golden/modes_<set>.npz hold the reference's own leaves ranked per conformer
(tests/golden/make_golden_modes.py); the NumPy restatement - `explain_ref.tree_leaves` ranked by `modes_ref.ranked_modes` - must
reproduce them, the CPU model of the MODES walker must lose no mode to its drops, and the interface must be declared where it belongs."""

import re

import numpy as np
import pytest

from conftest import GOLDEN, REPO, load_golden
from constrained_ref import random_constraint
from explain_ref import NONE, Tables, candidates, ligand_levels, path_score, tree_leaves
from modes_ref import MAX_MODES, MODES_SETS, completion_bounds, fixture_rows, key_exact, load_modes, ranked_modes, walk_modes_with_drops


@pytest.mark.parametrize("name", MODES_SETS)
def test_restated_tree_reproduces_the_reference_modes(name):
    """Rows whose tree has at most 2000 nodes: values within 2e-6 (the float64-restatement bar of test_explain_cpu.py), as many entries as
    the reference has, keys equal where the entry's own gap and its predecessor's exceed 1e-5 (else a key whose path_score is the value)."""
    from pharmaconet_amd.constants import weights_vector

    model, lib, weights, d, x = load_modes(name)
    w7 = weights_vector(weights)
    exact = rows = 0
    for i, C, lv, values, key, gap, n_positive in fixture_rows(x):
        assert (np.diff(values, axis=0) <= 0).all() and ((values > 0).sum(axis=0) == np.minimum(n_positive, MAX_MODES)).all()
        if d["n_tree"][i] > 2000:
            continue
        rec = lib.unpack(i)
        T = Tables(model, rec, w7)
        levels, leaves = tree_leaves(model, rec, w7, T)
        assert levels == lv.tolist()
        got, keys = ranked_modes(leaves, C, MAX_MODES)
        assert np.allclose(got, values, rtol=2e-6, atol=0), (name, i)
        rows += 1
        for m in range(MAX_MODES):
            for c in range(C):
                if values[m, c] <= 0:
                    assert keys[m][c] is None and (key[m, c] == NONE).all()
                elif key_exact(gap, m, c):
                    assert keys[m][c] == tuple(key[m, c].tolist()), (name, i, m, c)
                    exact += 1
                else:
                    assert abs(path_score(model, rec, w7, lv, keys[m][c], c, T) - values[m, c]) <= 2e-6 * values[m, c]
    assert rows > 0 and exact > 0


@pytest.mark.parametrize("name", MODES_SETS)
def test_fixture_rows_bite(name):
    """What the generator asserted when it minted the file: a conformer with more than one and fewer than 8 leaves, one with at least 8,
    and at most half of the positive entries within 1e-5 of a neighbour (those are compared by total, not by key). set_s64_c8 and
    set_l110_c8 have no ligand with such a short list - the generator ranks every ligand of theirs up to 30 000 nodes and asserts it
    (shortest lists: 9 and 42 leaves) - so there the short list is not asked for."""
    _, _, _, _, x = load_modes(name)
    few = many = loose = positive = 0
    for i, C, lv, values, key, gap, n_positive in fixture_rows(x):
        few += bool(((n_positive > 1) & (n_positive < MAX_MODES)).any())
        many += bool((n_positive >= MAX_MODES).any())
        for m in range(MAX_MODES):
            for c in range(C):
                if values[m, c] > 0:
                    positive += 1
                    loose += not key_exact(gap, m, c)
    assert (few > 0 or name in ("set_s64_c8", "set_l110_c8")) and many > 0 and 2 * loose <= positive
    if (GOLDEN / f"explain_{name}.npz").exists():  # mode 0 is that fixture's answer on the rows they share
        e = np.load(GOLDEN / f"explain_{name}.npz")
        shared = [(r, int(np.flatnonzero(e["index"] == i)[0])) for r, i in enumerate(x["index"]) if i in e["index"]]
        assert shared
        for r, q in shared:
            assert np.array_equal(x["values"][r, 0], e["scores"][q]) and np.array_equal(x["key"][r, 0], e["key"][q])


@pytest.mark.parametrize("name", MODES_SETS)
def test_walker_model_loses_no_mode(name):
    """The 12 smallest trees of the set, M in 1, 2, 8, without and with seeded random constraints: the MODES walker's rule - enter above
    the M-th value, drop below it - gives exactly the ranked leaves of the full tree, under the tightest admissible bound."""
    from pharmaconet_amd.constants import weights_vector

    model, lib, weights, d = load_golden(name)
    w7 = weights_vector(weights)
    rng = np.random.default_rng(7)
    idx = [int(i) for i in np.argsort(d["n_tree"], kind="stable") if 3 <= d["n_tree"][i] <= 2000][:12]
    assert idx
    positive = 0
    for i in idx:
        rec = lib.unpack(i)
        T = Tables(model, rec, w7)
        lv, leaves = tree_leaves(model, rec, w7, T)
        R = completion_bounds(model, rec, T)
        cand = sorted({m for lc in ligand_levels(model, rec) for m in candidates(model, rec, lc)})
        for M in (1, 2, 8):
            for require, exclude in (((), ()), random_constraint(rng, cand, model.flat.num_clusters)):
                want, want_keys = ranked_modes(leaves, T.C, M, require, exclude)
                got, keys, _ = walk_modes_with_drops(model, rec, w7, M, require, exclude, T, R)
                assert np.array_equal(got, want) and keys == want_keys, (name, i, M, require, exclude)
                positive += int((want > 0).any())
    assert positive > 0


def test_drops_fire_and_change_nothing():
    """A tree with leaves of five matches and more: the bound drops subtrees (fewer nodes walked than the tree has), more of them for
    fewer modes, and the modes stay those of the full tree."""
    from pharmaconet_amd.constants import weights_vector

    model, lib, weights, d = load_golden("set_c21_c8")
    w7 = weights_vector(weights)
    i = None
    for j in np.argsort(d["n_tree"], kind="stable"):  # the first tree of that size whose leaves reach six matches
        if 500 <= d["n_tree"][j] <= 6000:
            _, leaves = tree_leaves(model, lib.unpack(int(j)), w7)
            if any(sum(m != NONE for m in k) >= 6 for k, _ in leaves):
                i = int(j)
                break
    assert i is not None
    rec = lib.unpack(i)
    T = Tables(model, rec, w7)
    _, leaves = tree_leaves(model, rec, w7, T)
    R = completion_bounds(model, rec, T)
    walked = {}
    for M in (1, 8):
        want, want_keys = ranked_modes(leaves, T.C, M)
        got, keys, walked[M] = walk_modes_with_drops(model, rec, w7, M, tables=T, bounds=R)
        assert np.array_equal(got, want) and keys == want_keys
    assert walked[1] <= walked[8] < int(d["n_tree"][i])


def test_ranking_on_a_made_up_tie():
    leaves = [([0, NONE], {0: 1.0, 1: 2.0}), ([1, 2], {0: 3.0}), ([1, NONE], {0: 3.0, 1: 2.0}), ([NONE, 2], {1: 5.0}), ([2, 2], {0: 3.0, 1: 0.0})]
    values, keys = ranked_modes(leaves, 3, 3)
    assert values.T.tolist() == [[3.0, 3.0, 3.0], [5.0, 2.0, 2.0], [0.0, 0.0, 0.0]]
    assert [k[0] for k in keys] == [(1, 2), (1, NONE), (2, 2)]  # equal scores: iteration order
    assert [k[1] for k in keys] == [(NONE, 2), (0, NONE), (1, NONE)] and [k[2] for k in keys] == [None] * 3  # (a score of 0 is no mode)
    values, keys = ranked_modes(leaves, 3, 2, [[2]], [])
    assert values.T.tolist() == [[3.0, 3.0], [5.0, 0.0], [0.0, 0.0]] and [k[0] for k in keys] == [(1, 2), (2, 2)]
    values, keys = ranked_modes(leaves, 3, 8)
    assert (values[:, 0] > 0).sum() == 4 and values[3, 0] == 1.0 and keys[4][0] is None


def test_declared_in_header_and_binding():
    from pharmaconet_amd import _ffi

    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "pmx.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+pmx_explain_modes\s*\(", text) and re.search(r"#define\s+PMX_MAX_MODES\s+8\b", text)
    restype, argtypes = _ffi.SIGNATURES["pmx_explain_modes"]
    assert len(argtypes) == 13 and _ffi.MAX_MODES == MAX_MODES


def test_cli_usage_errors(tmp_path):
    from pharmaconet_amd.screening import Screening_ArgParser, main

    args = ["-p", str(GOLDEN / "model_6oim_like.pm"), "-d", str(tmp_path / "none.pmxlib"), "-o", str(tmp_path / "out.csv")]
    ns = Screening_ArgParser().parse_args(args + ["--explain", "5", "--modes", "3"])
    assert ns.modes == 3 and ns.modes_out is None
    for misuse in (["--modes", "3"], ["--explain", "5", "--modes", "0"], ["--explain", "5", "--modes", "9"], ["--explain", "5", "--modes_out", "x.csv"]):
        with pytest.raises(SystemExit) as err:
            main(args + misuse)
        assert err.value.code == 2
    assert not (tmp_path / "out.csv").exists()
