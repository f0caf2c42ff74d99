"""`pmx_explain_modes` on the GPU (csrc/pmx_explain.hip: the one explain walker, here with M modes): per conformer the best leaves of the reference's tree, checked
against the reference's own ranked leaves (tests/golden/modes_<set>.npz), `explain` (mode 0, bit for bit), the NumPy restatement
(tests/modes_ref.py) and `attribute`."""

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from constrained_ref import qualifies, random_constraint
from explain_ref import Tables, candidates, ligand_levels, path_score, tree_leaves
from modes_ref import MAX_MODES, MODES_SETS, fixture_rows, key_exact, load_modes, ranked_modes

pytestmark = pytest.mark.gpu


def same_mode(ms, r, m, ex, q):
    """Mode m of row r of a ModeSet and row q of an Explanation (or mode m of another ModeSet's row q) hold the same bits."""
    other = ex.explanation(m) if hasattr(ex, "explanation") else ex
    return (np.array_equal(ms.values[r][m], other.conf_max[q], equal_nan=True) and np.array_equal(ms.match[r][m], other.match[q])
            and np.array_equal(ms.levels[r], other.levels[q]) and ms.best_conformer[r] == other.best_conformer[q] and ms.status[r] == other.status[q])


def most_matched(ex, K):
    count = np.zeros(K, np.int64)
    for m in ex.match:
        count[m[m >= 0]] += 1
    return [int(a) for a in np.argsort(-count, kind="stable") if count[a] > 0]


@pytest.mark.parametrize("name", MODES_SETS)
def test_reference_modes_fixtures(name):
    """The reference's own ranked leaves: status 0, levels exact, values within 2e-6 (test_gpu_explain.py's bar for the tabulated functions),
    keys exact where the entry's own gap and its predecessor's exceed 1e-5 (else a key whose path_score is the reference value within
    2e-6), entries beyond n_positive 0 / -1."""
    from pharmaconet_amd.constants import weights_vector
    from pharmaconet_amd.engine import DeviceLibrary, explain_modes

    model, lib, weights, _, x = load_modes(name)
    w7 = weights_vector(weights)
    rows = list(fixture_rows(x))
    ms = explain_modes(model, DeviceLibrary(lib), [r[0] for r in rows], modes=MAX_MODES, weights=weights)
    exact = 0
    for r, (i, C, lv, values, key, gap, n_positive) in enumerate(rows):
        assert ms.status[r] == 0 and ms.levels[r].tolist() == lv.tolist()
        print(name, i, "max relative error", float(np.max(np.abs(ms.values[r] - values) / np.where(values > 0, values, 1.0))))
        assert np.allclose(ms.values[r], values, rtol=2e-6, atol=0), (name, i)
        assert ms.best_conformer[r] == int(np.argmax(values[0])) and ms.count(r).tolist() == np.minimum(n_positive, MAX_MODES).tolist()
        T = None
        for m in range(MAX_MODES):
            for c in range(C):
                got = ms.match[r][m, c]
                if m >= n_positive[c]:
                    assert ms.values[r][m, c] == 0 and (got == -1).all()
                elif key_exact(gap, m, c):
                    assert got.tolist() == key[m, c].tolist(), (name, i, m, c)
                    exact += 1
                else:
                    if T is None:
                        rec = lib.unpack(i)
                        T = Tables(model, rec, w7)
                    assert abs(path_score(model, rec, w7, lv, got, c, T) - values[m, c]) <= 2e-6 * values[m, c], (name, i, m, c)
    assert exact > 0


@pytest.mark.parametrize("name", ("set_c21_c8", "set_6oim_c64"))
def test_mode_0_is_explain(name):
    """modes=1 and mode 0 of modes=8 are `explain` bit for bit on every row, without a constraint and under one built from the most
    matched clusters; mode m of modes=3 is mode m of modes=8."""
    from pharmaconet_amd.engine import DeviceLibrary, explain, explain_modes

    model, lib, weights, _ = load_golden(name)
    dlib = DeviceLibrary(lib)
    idx = np.arange(len(lib))
    top = most_matched(explain(model, dlib, idx, weights=weights), model.flat.num_clusters)
    for con in ({}, dict(require=[[top[1], top[2]]], exclude=[top[0]])):
        base = explain(model, dlib, idx, weights=weights, **con)
        one = explain_modes(model, dlib, idx, modes=1, weights=weights, **con)
        three = explain_modes(model, dlib, idx, modes=3, weights=weights, **con)
        eight = explain_modes(model, dlib, idx, modes=8, weights=weights, **con)
        assert eight.require == base.require and eight.exclude == base.exclude
        for r in idx:
            assert same_mode(one, r, 0, base, r) and same_mode(eight, r, 0, base, r), (name, con, r)
            assert all(same_mode(three, r, m, eight, r) for m in range(3)), (name, con, r)
        assert any(c.max() > 1 for c in map(eight.count, idx) if c.size)


def test_structure_on_synthetic_ligands():
    """512 synthetic ligands, M = 8: values non-increasing, keys pairwise distinct, equal neighbours in key order (None last), pmx_attribute's
    total of every reported key at the best conformer is the mode's value (2e-6), and under a constraint every key qualifies and every
    constrained value is one of the unconstrained modes or lies below the unconstrained eighth."""
    from pharmaconet_amd.engine import DeviceLibrary, attribute, explain_modes
    from test_survey_library import _model_nodes
    from tools.synthetic import synthetic_library

    model, _, _, _ = load_golden("set_6oim_c8")
    lib = synthetic_library(512, model_nodes=_model_nodes(model))
    dlib = DeviceLibrary(lib)
    idx = np.arange(len(lib))
    base = explain_modes(model, dlib, idx, modes=MAX_MODES)
    order = lambda k: [int(a) if a >= 0 else 1 << 20 for a in k]  # noqa: E731  (children in ascending cluster order, None last)
    rows, confs, keys, want = [], [], [], []
    ties = 0
    for r in idx:
        if base.status[r] != 0:
            assert np.isnan(base.values[r]).all() and base.best_conformer[r] == -1
            continue
        v, k = base.values[r], base.match[r]
        assert (np.diff(v, axis=0) <= 0).all()
        for c in range(v.shape[1]):
            found = int(base.count(r)[c])
            assert (v[found:, c] == 0).all() and (k[found:, c] == -1).all()
            assert len({tuple(k[m, c]) for m in range(found)}) == found
            for m in range(found - 1):
                if v[m, c] == v[m + 1, c]:
                    assert order(k[m, c]) < order(k[m + 1, c]), (r, c, m)
                    ties += 1
            if c == base.best_conformer[r]:
                for m in range(found):
                    rows.append(r), confs.append(c), keys.append(k[m, c]), want.append(v[m, c])
    assert max(int(base.count(r).max()) for r in idx if base.status[r] == 0 and base.values[r].size) == MAX_MODES
    want = np.array(want)
    for lo in range(0, len(rows), 65536):
        at = attribute(model, dlib, rows[lo : lo + 65536], confs[lo : lo + 65536], keys[lo : lo + 65536])
        assert (at.status == 0).all() and (np.abs(at.total - want[lo : lo + 65536]) <= 2e-6 * want[lo : lo + 65536]).all()
    used = most_matched(base.explanation(0), model.flat.num_clusters)
    changed = 0
    for require, exclude in (([[used[0]]], []), ([], [used[0]]), ([[used[-1], used[1]]], [used[2]])):
        ms = explain_modes(model, dlib, idx, modes=MAX_MODES, require=require, exclude=exclude)
        assert np.array_equal(ms.status, base.status)
        for r in idx:
            if base.status[r] != 0:
                continue
            for c in range(ms.values[r].shape[1]):
                for m in range(int(ms.count(r)[c])):
                    assert qualifies(ms.match[r][m, c], require, exclude), (r, c, m, require, exclude)
                    v = ms.values[r][m, c]
                    assert v in base.values[r][:, c] or v < base.values[r][MAX_MODES - 1, c], (r, c, m)
                changed += not np.array_equal(ms.values[r][:, c], base.values[r][:, c])
    assert changed > 0


@pytest.mark.parametrize("name", MODES_SETS)
def test_restated_tree_with_random_constraints(name):
    """The 12 smallest trees of the set under seeded random constraints, M in (2, 8), against the restated tree's ranked leaves: values
    within 2e-6, as many modes, keys equal or - where the restatement's float64 totals order near ties otherwise - of the same total."""
    from pharmaconet_amd.constants import weights_vector
    from pharmaconet_amd.engine import DeviceLibrary, explain_modes

    model, lib, weights, d = load_golden(name)
    dlib = DeviceLibrary(lib)
    w7 = weights_vector(weights)
    rng = np.random.default_rng(11)
    idx = [int(i) for i in np.argsort(d["n_tree"], kind="stable") if d["n_tree"][i] <= 2000][:12]
    exact = positive = 0
    for i in idx:
        rec = lib.unpack(i)
        T = Tables(model, rec, w7)
        lv, leaves = tree_leaves(model, rec, w7, T)
        cand = sorted({m for lc in ligand_levels(model, rec) for m in candidates(model, rec, lc)})
        for M in (2, 8):
            require, exclude = random_constraint(rng, cand, model.flat.num_clusters)
            want, keys = ranked_modes(leaves, T.C, M, require, exclude)
            ms = explain_modes(model, dlib, [i], modes=M, weights=weights, require=require, exclude=exclude)
            assert ms.status[0] == 0 and ms.levels[0].tolist() == list(lv)
            assert np.allclose(ms.values[0], want, rtol=2e-6, atol=0), (name, i, M, require, exclude)
            positive += int((want > 0).any())
            for m in range(M):
                for c in range(T.C):
                    got = ms.match[0][m, c]
                    if want[m, c] <= 0:
                        assert (got == -1).all()
                        continue
                    assert qualifies(got, require, exclude)
                    if tuple(int(a) for a in got) == keys[m][c]:
                        exact += 1
                    else:
                        assert abs(path_score(model, rec, w7, lv, got, c, T) - want[m, c]) <= 2e-6 * want[m, c], (name, i, M, m, c)
    assert exact > 0 and positive > 0


def test_invariance_and_two_streams(monkeypatch):
    """As test_gpu_explain.py's: the same bits through the overflow passes, under permutation and repeats, and from two threads on two streams."""
    import threading

    import torch

    from pharmaconet_amd.engine import DeviceLibrary, explain_modes, last_score_stats, release_workspaces, screen

    model, lib, weights, _ = load_golden("set_c21_c8")
    dlib = DeviceLibrary(lib)
    n = len(lib)
    base = explain_modes(model, dlib, np.arange(n), modes=MAX_MODES, weights=weights)
    assert max(int(base.count(r).max()) for r in range(n) if base.values[r].size) == MAX_MODES

    def same(ms, rows):
        for r, i in enumerate(rows):
            assert all(same_mode(ms, r, m, base, i) for m in range(MAX_MODES)), (r, i)

    for env in ({"PMX_SLICE_KB": "8"}, {"PMX_SLICE_KB": "8", "PMX_BIG_SLICE_MB": "1", "PMX_BIG_TOTAL_MB": "64"}):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            same(explain_modes(model, dlib, np.arange(n), modes=MAX_MODES, weights=weights), np.arange(n))
            screen(model, dlib, weights=weights, float64=True)
            assert last_score_stats()["n_slice_overflow"] > 0, env  # the setting does reach the overflow passes
    rng = np.random.default_rng(3)
    perm = rng.permutation(n)
    same(explain_modes(model, dlib, perm, modes=MAX_MODES, weights=weights), perm)
    sub = perm[:17]
    rep = np.concatenate([sub, sub[::-1], sub[:3]])
    same(explain_modes(model, dlib, rep, modes=MAX_MODES, weights=weights), rep)
    out = {}

    def run(k):
        with torch.cuda.stream(torch.cuda.Stream()):
            out[k] = explain_modes(model, dlib, perm, modes=MAX_MODES, weights=weights)

    ts = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    same(out[0], perm)
    same(out[1], perm)
    release_workspaces()  # (the two streams' workspaces hold an arena each: handed back for the large-library tests that follow)


def test_edge_cases():
    from pharmaconet_amd import PackedLibrary
    from pharmaconet_amd._ffi import PmxError
    from pharmaconet_amd.engine import DeviceLibrary, _explain_rows, explain, explain_modes
    from pharmaconet_amd.library import UNSUPPORTED_RECORD, LigandFeatures, pack_ligand

    model, lib, _, _ = load_golden("set_c21_c8")
    for bad in (0, 9):
        with pytest.raises(PmxError):
            explain_modes(model, lib, [0, 1], modes=bad)
    with pytest.raises(PmxError):
        explain_modes(model, lib, [0], require=[[model.flat.num_clusters]])
    zero = pack_ligand(LigandFeatures([6, 8], [[1], [0]], [], np.zeros((2, 4, 3), np.float32)))
    hal = pack_ligand(LigandFeatures([6, 17], [[1], [0]], [("Halogen", 1, 1)], np.ones((2, 4, 3), np.float32)))
    small = PackedLibrary.from_records([zero, hal, UNSUPPORTED_RECORD, lib.record(0)])
    dsmall = DeviceLibrary(small)
    # n * modes beyond PMX_EXPLAIN_MAX: the engine cuts the list, the call itself refuses
    many = np.full(65536 // 8 + 5, 3)
    with pytest.raises(PmxError):
        _explain_rows(model, dsmall, many, 8, None, None, "pmx_explain_modes")
    ms = explain_modes(model, dsmall, many, modes=8)
    assert len(ms) == len(many) and all(same_mode(ms, r, m, ms, 0) for r in (1, len(many) // 2, len(many) - 1) for m in range(8))
    plain = explain(model, dsmall, [3])
    assert same_mode(ms, len(many) - 1, 0, plain, 0)
    ms = explain_modes(model, dsmall, [0, 1, 2, 3, 4], modes=3)
    assert ms.status.tolist() == [0, 0, 1, 0, 1]  # (index 4 is outside the library)
    for r in (0, 1):
        assert ms.values[r].shape == (3, 4) and (ms.values[r] == 0).all() and ms.match[r].size == 0 and ms.best_conformer[r] == 0 and (ms.count(r) == 0).all()
    for r in (2, 4):
        assert ms.values[r].shape == (3, 1) and np.isnan(ms.values[r]).all() and ms.best_conformer[r] == -1
    assert explain_modes(model, dsmall, [], modes=3).indices.size == 0
    # infeasible: a cluster required alone and excluded - status 0, all modes 0, no keys
    a = int(plain.match[0][plain.best_conformer[0]].max())
    ms = explain_modes(model, dsmall, [3, 3], modes=4, require=[[a]], exclude=[a])
    for r in range(2):
        assert ms.status[r] == 0 and ms.best_conformer[r] == 0 and (ms.values[r] == 0).all() and (ms.match[r] == -1).all()
        assert ms.values[r].shape == (4, len(plain.conf_max[0])) and ms.levels[r].tolist() == plain.levels[0].tolist()
    det = model.scoring_modes(lib.record(0), modes=5, exclude=[a])
    one = explain_modes(model, dsmall, [3], modes=5, exclude=[a])
    assert np.array_equal(det["values"], one.values[0]) and np.array_equal(det["match"], one.match[0]) and det["best_conformer"] == one.best_conformer[0]
    assert len(det["pairs"]) == det["count"][det["best_conformer"]] and one.gap(0) == one.gap(0, int(one.best_conformer[0]), 0)
    v = one.values[0][:, one.best_conformer[0]]
    assert one.gap(0, m=1) == ((v[1] - v[2]) / v[1] if v[2] > 0 else 1.0)
    with pytest.raises(ValueError):
        one.gap(0, m=4)
    res = model.screen(lib, topk=4)
    assert np.array_equal(res.modes(4, modes=2).values[1], model.explain_modes(lib, [res.ranking()[1][0]], modes=2).values[0])


def test_cli(tmp_path, capsys):
    from pharmaconet_amd.screening import main

    _, lib, _, _ = load_golden("set_6oim_c1")
    libfile = tmp_path / "lib.pmxlib"
    lib.save(libfile)
    args = ["-p", str(GOLDEN / "model_6oim_like.pm"), "-d", str(libfile)]
    main(args + ["-o", str(tmp_path / "plain.csv"), "--explain", "5"])
    main(args + ["-o", str(tmp_path / "with.csv"), "--explain", "5", "--modes", "3"])
    assert (tmp_path / "plain.csv").read_bytes() == (tmp_path / "with.csv").read_bytes()
    assert (tmp_path / "plain.csv.explain.csv").read_bytes() == (tmp_path / "with.csv.explain.csv").read_bytes()
    rows = (tmp_path / "with.csv.modes.csv").read_text().splitlines()
    assert rows[0] == "rank,path,mode,mode_score,fraction_of_best,matches"
    explained = [r.split(",") for r in (tmp_path / "with.csv.explain.csv").read_text().splitlines()[1:]]
    per_hit = {}
    for row in rows[1:]:
        f = row.split(",")
        per_hit.setdefault(int(f[0]), []).append(f)
    assert sorted(per_hit) == [int(e[0]) for e in explained] and max(len(v) for v in per_hit.values()) > 1
    for e in explained:
        got = per_hit[int(e[0])]
        assert [int(f[2]) for f in got] == list(range(len(got))) and len(got) <= 3 and all(f[1] == e[1] and f[5] for f in got)
        scores = [float(f[3]) for f in got]
        assert scores[0] == float(e[4]) and got[0][5] == e[5] and float(got[0][4]) == 1.0  # mode 0 is the explain CSV's maximum and match
        assert (np.diff(scores) <= 0).all() and all(abs(float(f[4]) - float(f[3]) / scores[0]) < 1e-12 for f in got)
    main(args + ["-o", str(tmp_path / "to.csv"), "--explain", "2", "--modes", "2", "--modes_out", str(tmp_path / "m.csv")])
    assert (tmp_path / "m.csv").exists() and not (tmp_path / "to.csv.modes.csv").exists()
    capsys.readouterr()
