"""CPU side of constrained matching (`pmx_explain_constrained`): tests/golden/constrained_<set>.npz hold the reference's own leaves
filtered by a constraint (tests/golden/make_golden_constrained.py); the NumPy restatement - `explain_ref.tree_leaves` filtered by
`constrained_ref.constrained_first_max_key` - must reproduce them, and the Python layer must normalise constraints as documented."""

import numpy as np
import pytest

from conftest import GOLDEN
from constrained_ref import CONSTRAINED_SETS, constrained_first_max_key, fixture_rows, load_constrained, qualifies
from explain_ref import NONE, Tables, path_score, tree_leaves


@pytest.mark.parametrize("name", CONSTRAINED_SETS)
def test_restated_tree_reproduces_the_reference_under_constraints(name):
    """Rows whose tree has at most 2000 nodes: maxima within 2e-6 (the tolerance of the explain tests against the reference), keys equal
    where the runner-up with another qualifying key is more than 1e-5 below."""
    from pharmaconet_amd.constants import weights_vector

    model, lib, weights, d, x = load_constrained(name)
    w7 = weights_vector(weights)
    trees = {}
    exact = rows = 0
    for i, kind, C, lv, require, exclude, sc, key, gap, unc in fixture_rows(x):
        assert (sc <= unc).all()
        if d["n_tree"][i] > 2000:
            continue
        if i not in trees:
            rec = lib.unpack(i)
            T = Tables(model, rec, w7)
            trees[i] = (rec, T, tree_leaves(model, rec, w7, T))
        rec, T, (levels, leaves) = trees[i]
        assert levels == lv.tolist()
        best, keys = constrained_first_max_key(leaves, C, require, exclude)
        assert np.allclose(best, sc, rtol=2e-6, atol=0), (name, i, kind)
        rows += 1
        for c in range(C):
            if sc[c] <= 0:
                assert keys[c] is None and (key[c] == NONE).all()
                continue
            assert qualifies(key[c], require, exclude) and qualifies(keys[c], require, exclude)
            if gap[c] > 1e-5:
                assert keys[c] == tuple(key[c].tolist()), (name, i, kind, c)
                exact += 1
            else:
                assert abs(path_score(model, rec, w7, lv, keys[c], c, T) - sc[c]) <= 2e-6 * sc[c]
    assert rows > 0 and exact > 0


@pytest.mark.parametrize("name", CONSTRAINED_SETS)
def test_fixture_rows_bite(name):
    """What the generator asserted when it minted the file: constraints change the answer on at least half of the exclude (b) and foreign
    require (c) rows while something still scores, (a) leaves the best conformer's maximum alone, (e) leaves nothing."""
    _, _, _, _, x = load_constrained(name)
    rows = list(fixture_rows(x))
    for kind in "bc":
        rk = [r for r in rows if r[1] == kind]
        assert rk and 2 * sum(1 for r in rk if not np.array_equal(r[6], r[9]) and r[6].max() > 0) >= len(rk)
    for i, kind, C, lv, require, exclude, sc, key, gap, unc in rows:
        if kind == "a":
            assert sc[int(np.argmax(unc))] == unc.max()
        if kind == "d":
            assert len(require) == 2 and len(require[0]) == 2
        if kind == "e":
            assert (sc == 0).all() and (key == NONE).all()
    if name == "set_l110_c8":
        assert any(r[1] == "b" and r[5][0] >= 64 for r in rows) and any(r[1] == "c" and r[4][0][0] >= 64 for r in rows)


def test_constraint_rule_on_made_up_leaves():
    leaves = [([0, NONE], {0: 1.0, 1: 2.0}), ([1, 2], {0: 3.0}), ([1, NONE], {0: 3.0, 1: 2.0}), ([NONE, 2], {1: 5.0})]
    best, keys = constrained_first_max_key(leaves, 3, [], [])
    assert best.tolist() == [3.0, 5.0, 0.0] and keys == [(1, 2), (NONE, 2), None]
    best, keys = constrained_first_max_key(leaves, 3, [[1]], [])
    assert best.tolist() == [3.0, 2.0, 0.0] and keys == [(1, 2), (1, NONE), None]
    best, keys = constrained_first_max_key(leaves, 3, [[0, 1]], [2])
    assert best.tolist() == [3.0, 2.0, 0.0] and keys == [(1, NONE), (0, NONE), None]
    best, keys = constrained_first_max_key(leaves, 3, [[0], [2]], [])
    assert best.tolist() == [0.0, 0.0, 0.0] and keys == [None, None, None]
    best, keys = constrained_first_max_key(leaves, 3, [[2]], [2])  # required alone and excluded: infeasible, not an error
    assert best.tolist() == [0.0, 0.0, 0.0]


def test_argument_normalisation():
    from pharmaconet_amd import _ffi
    from pharmaconet_amd.engine import _constraint_struct, key_qualifies, normalize_constraint

    assert normalize_constraint(None, None) == ((), ())
    assert normalize_constraint([3, [5, 2, 5], (7,)], [9, 1, 9]) == (((3,), (2, 5), (7,)), (1, 9))
    assert normalize_constraint([np.int64(4), np.array([70, 1])], np.array([65])) == (((4,), (1, 70)), (65,))
    assert normalize_constraint([[]], None) == (((),), ())  # (an empty group is the C call's to refuse)
    for bad in (([-1], None), (None, [-2]), ([[1.5]], None), (["a"], None), ([True], None)):
        with pytest.raises(ValueError):
            normalize_constraint(*bad)
    with pytest.raises(ValueError):
        normalize_constraint([20], None, num_clusters=20)
    assert normalize_constraint([19], [0], num_clusters=20) == (((19,),), (0,))
    con = _constraint_struct(((3,), (1, 70)), (65, 127))
    assert con.n_require == 2 and ctypes_words(con.require[0]) == [1 << 3, 0] and ctypes_words(con.require[1]) == [1 << 1, 1 << 6]
    assert ctypes_words(con.exclude) == [0, (1 << 1) | (1 << 63)]
    assert ctypes_words(con.require[2]) == [0, 0] and _ffi.MAX_REQUIRE_GROUPS == 8
    assert key_qualifies([3, -1, 70], ((3,), (1, 70)), (65,)) and not key_qualifies([3, -1, 65, 70], ((3,), (1, 70)), (65,))
    assert not key_qualifies([3, -1], ((3,), (1, 70)), ())


def ctypes_words(w):
    return [int(w[0]), int(w[1])]


def test_clusters_with_nodes():
    from pharmaconet_amd import PharmacophoreModel
    from pharmaconet_amd.pharmacophore_model import cluster_node_sets

    model = PharmacophoreModel.load(GOLDEN / "model_6oim_like.pm")
    sets = cluster_node_sets(model.flat)
    seen = set()
    for m in range(model.flat.num_nodes):
        got = model.clusters_with_nodes([m])
        assert got == [a for a, s in enumerate(sets) if (s >> m) & 1] and got == model.clusters_with_nodes(m)
        seen.update(got)
    assert seen == set(range(model.flat.num_clusters))  # every cluster holds a node
    a = max(range(len(sets)), key=lambda k: bin(sets[k]).count("1"))
    members = [m for m in range(model.flat.num_nodes) if (sets[a] >> m) & 1]
    assert a in model.clusters_with_nodes(members) and model.clusters_with_nodes([]) == []
    assert model.clusters_with_nodes(members) == sorted(set().union(*[model.clusters_with_nodes(m) for m in members]))
    with pytest.raises(ValueError):
        model.clusters_with_nodes([model.flat.num_nodes])


@pytest.mark.parametrize("name", ("set_c21_c8", "set_6oim_c8", "set_l110_c8"))
def test_drop_rule_changes_no_answer(name):
    """The walker may leave out a child with >= 5 matches below which nothing can qualify (crediting it with one match): maxima and keys
    stay those of the full tree filtered by the constraint, on trees deep enough for the rule to fire."""
    from conftest import load_golden
    from constrained_ref import random_constraint, walk_with_drops
    from explain_ref import candidates, ligand_levels
    from pharmaconet_amd.constants import weights_vector

    model, lib, weights, d = load_golden(name)
    w7 = weights_vector(weights)
    rng = np.random.default_rng(5)
    idx = [int(i) for i in np.argsort(d["n_tree"], kind="stable") if 200 <= d["n_tree"][i] <= 6000][-4:]
    assert idx
    saved = 0
    for i in idx:
        rec = lib.unpack(i)
        T = Tables(model, rec, w7)
        lv, leaves = tree_leaves(model, rec, w7, T)
        cand = sorted({m for lc in ligand_levels(model, rec) for m in candidates(model, rec, lc)})
        for _ in range(4):
            require, exclude = random_constraint(rng, cand, model.flat.num_clusters)
            want, want_keys = constrained_first_max_key(leaves, T.C, require, exclude)
            best, keys, walked = walk_with_drops(model, rec, w7, require, exclude, T)
            assert np.array_equal(best, want) and keys == want_keys, (name, i, require, exclude)
            saved += walked < int(d["n_tree"][i])
    assert saved > 0
