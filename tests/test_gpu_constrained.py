"""`pmx_explain_constrained` on the GPU (csrc/pmx_explain.hip, the CONSTRAINED walker): per-conformer maxima and keys over the leaves
that qualify under a constraint, checked against the reference's filtered leaves (tests/golden/constrained_<set>.npz), the NumPy
restatement (tests/constrained_ref.py), the unconstrained walker, and - for `screen_constrained` - a brute-force ranking."""

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from constrained_ref import CONSTRAINED_SETS, constrained_first_max_key, fixture_rows, load_constrained, qualifies, random_constraint
from explain_ref import Tables, candidates, ligand_levels, path_score, tree_leaves

pytestmark = pytest.mark.gpu


def same_rows(a, ra, b, rb):
    """Row ra of explanation a and row rb of b hold the same bits."""
    return (np.array_equal(a.conf_max[ra], b.conf_max[rb], equal_nan=True) and np.array_equal(a.match[ra], b.match[rb])
            and np.array_equal(a.levels[ra], b.levels[rb]) and a.best_conformer[ra] == b.best_conformer[rb] and a.status[ra] == b.status[rb])


def check_row(model, lib, w7, ex, r, i, C, lv, require, exclude, sc, keys, gap):
    """One explained row against reference maxima `sc` and keys (a tuple / array per conformer, None or all -1 for no key): the bars of
    test_gpu_explain.py. Returns how many keys were compared exactly."""
    assert ex.status[r] == 0
    assert np.allclose(ex.conf_max[r], sc, rtol=2e-6, atol=0), (i, require, exclude, ex.conf_max[r], sc)
    assert ex.levels[r].tolist() == list(lv)
    assert ex.best_conformer[r] == int(np.argmax(sc))
    exact, T = 0, None
    for c in range(C):
        got = ex.match[r][c]
        if sc[c] <= 0:
            assert (got == -1).all()
            continue
        assert qualifies(got, require, exclude), (i, c, got.tolist(), require, exclude)  # every reported key qualifies
        if gap[c] > 1e-5:
            assert got.tolist() == [int(m) for m in keys[c]], (i, c, require, exclude)
            exact += 1
        else:
            if T is None:
                rec = lib.unpack(i)
                T = Tables(model, rec, w7)
            assert abs(path_score(model, rec, w7, lv, got, c, T) - sc[c]) <= 2e-6 * sc[c], (i, c)
    return exact


@pytest.mark.parametrize("name", CONSTRAINED_SETS)
def test_reference_constrained_fixtures(name):
    """The reference's own leaves filtered by each row's constraint: status 0, maxima within 2e-6, levels and best conformer exact, the
    key exact where the runner-up among qualifying leaves is more than 1e-5 below (else a key whose path_score is the maximum), and
    every reported key qualifies."""
    from pharmaconet_amd.constants import weights_vector
    from pharmaconet_amd.engine import DeviceLibrary, explain

    model, lib, weights, _, x = load_constrained(name)
    dlib = DeviceLibrary(lib)
    w7 = weights_vector(weights)
    exact = 0
    for i, kind, C, lv, require, exclude, sc, key, gap, unc in fixture_rows(x):
        ex = explain(model, dlib, [i], weights=weights, require=require, exclude=exclude)
        assert ex.require == tuple(tuple(g) for g in require) and ex.exclude == tuple(exclude)
        exact += check_row(model, lib, w7, ex, 0, i, C, lv, require, exclude, sc, key, gap)
        assert abs(ex.scores[0] - sc.mean()) <= 2e-6 * sc.mean()
    assert exact > 0


@pytest.mark.parametrize("name", ("set_c21_c8", "set_6oim_c64"))
def test_empty_constraint_is_pmx_explain(name):
    """No constraint through pmx_explain_constrained (a NULL constraint: the unconstrained kernels; an empty one: the constrained
    kernels with nothing to test) is bit for bit pmx_explain, on every row of the set."""
    from pharmaconet_amd.engine import DeviceLibrary, _explain_rows, explain

    model, lib, weights, _ = load_golden(name)
    dlib = DeviceLibrary(lib)
    idx = np.arange(len(lib))
    base = explain(model, dlib, idx, weights=weights)
    assert base.require is None and base.exclude is None
    null = _explain_rows(model, dlib, idx, 1, weights, None, "pmx_explain_constrained").explanation()
    empty = explain(model, dlib, idx, weights=weights, require=[], exclude=[])
    assert empty.require == () and empty.exclude == ()
    for r in idx:
        assert same_rows(null, r, base, r) and same_rows(empty, r, base, r), (name, r)
    assert np.array_equal(base.scores, empty.scores, equal_nan=True)
    ok = base.status == 0
    assert ok.any() and np.array_equal(base.scores[ok], np.array([m.mean() for m, s in zip(base.conf_max, base.status) if s == 0]))
    assert np.isnan(base.scores[~ok]).all()


def test_dominance_on_synthetic_ligands():
    """512 synthetic ligands, constraints from the most and least matched clusters of their unconstrained explanation: a constrained
    maximum is never above the unconstrained one; where the unconstrained key qualifies, maximum and key are identical; where a
    constrained maximum is > 0 its key qualifies and pmx_attribute's total of that key is the maximum (2e-6, test_gpu_attribution.py)."""
    from pharmaconet_amd.engine import DeviceLibrary, attribute, explain
    from test_survey_library import _model_nodes
    from tools.synthetic import synthetic_library

    model, _, _, _ = load_golden("set_6oim_c8")
    lib = synthetic_library(512, model_nodes=_model_nodes(model))
    dlib = DeviceLibrary(lib)
    idx = np.arange(len(lib))
    base = explain(model, dlib, idx)
    K = model.flat.num_clusters
    count = np.zeros(K, np.int64)
    for r in idx:
        if base.status[r] == 0:
            for key in base.match[r]:
                count[key[key >= 0]] += 1
    used = [int(a) for a in np.argsort(-count, kind="stable") if count[a] > 0]
    assert len(used) >= 3
    most, least = used[0], used[-1]
    cases = (([[most]], []), ([], [most]), ([[least]], []), ([[least, used[1]], [most]], [used[2]]), ([], [least, used[1]]))
    changed = kept = attributed = 0
    for require, exclude in cases:
        ex = explain(model, dlib, idx, require=require, exclude=exclude)
        assert np.array_equal(ex.status, base.status)
        rows, confs, keys, want = [], [], [], []
        for r in idx:
            if base.status[r] != 0:
                assert np.isnan(ex.conf_max[r]).all() and ex.best_conformer[r] == -1
                continue
            assert np.array_equal(ex.levels[r], base.levels[r])
            assert (ex.conf_max[r] <= base.conf_max[r]).all(), (r, require, exclude)
            for c in range(len(base.conf_max[r])):
                uk, ck = base.match[r][c], ex.match[r][c]
                if base.conf_max[r][c] > 0 and qualifies(uk, require, exclude):
                    assert ex.conf_max[r][c] == base.conf_max[r][c] and np.array_equal(ck, uk), (r, c, require, exclude)
                    kept += 1
                elif ex.conf_max[r][c] != base.conf_max[r][c]:
                    changed += 1
                if ex.conf_max[r][c] > 0:
                    assert qualifies(ck, require, exclude), (r, c, ck.tolist(), require, exclude)
                    if c == ex.best_conformer[r]:
                        rows.append(r), confs.append(c), keys.append(ck), want.append(ex.conf_max[r][c])
                else:
                    assert (ck == -1).all()
        at = attribute(model, dlib, rows, confs, keys)
        want = np.array(want)
        assert (at.status == 0).all() and (np.abs(at.total - want) <= 2e-6 * want).all()
        attributed += len(rows)
    assert changed > 0 and kept > 0 and attributed > 0


@pytest.mark.parametrize("name", CONSTRAINED_SETS)
def test_restated_tree_with_random_constraints(name):
    """The 12 smallest trees (<= 2000 nodes) of the set under seeded random constraints - one and two groups of 1 - 3 clusters, exclude
    sets, cluster indices >= 64 on the large model - against the restated tree filtered by the constraint."""
    from pharmaconet_amd.constants import weights_vector
    from pharmaconet_amd.engine import DeviceLibrary, explain

    model, lib, weights, d = load_golden(name)
    dlib = DeviceLibrary(lib)
    w7 = weights_vector(weights)
    K = model.flat.num_clusters
    rng = np.random.default_rng(11)
    idx = [int(i) for i in np.argsort(d["n_tree"], kind="stable") if d["n_tree"][i] <= 2000][:12]
    assert idx
    exact = positive = high = 0
    for i in idx:
        rec = lib.unpack(i)
        T = Tables(model, rec, w7)
        lv, leaves = tree_leaves(model, rec, w7, T)
        cand = sorted({m for lc in ligand_levels(model, rec) for m in candidates(model, rec, lc)})
        for _ in range(4):
            require, exclude = random_constraint(rng, cand, K)
            high += any(a >= 64 for g in require for a in g) or any(a >= 64 for a in exclude)
            best, keys = constrained_first_max_key(leaves, T.C, require, exclude)
            ex = explain(model, dlib, [i], weights=weights, require=require, exclude=exclude)
            # (no gap is recorded here: a key that differs must still reproduce the maximum, as test_keys_are_the_first_leaf_of_the_restated_tree has it)
            gap = np.array([1.0 if keys[c] is not None and tuple(int(m) for m in ex.match[0][c]) == keys[c] else 0.0 for c in range(T.C)])
            exact += check_row(model, lib, w7, ex, 0, i, T.C, lv, require, exclude, best, keys, gap)
            positive += int((best > 0).any())
    assert exact > 0 and positive > 0
    if name == "set_l110_c8":
        assert high > 0


def test_invariance_and_two_streams(monkeypatch):
    """As test_gpu_explain.py's: the same bits through the overflow passes, under permutation and repeats, and from two threads on two streams."""
    import threading

    import torch

    from pharmaconet_amd.engine import DeviceLibrary, explain, last_score_stats, screen

    model, lib, weights, _ = load_golden("set_c21_c8")
    dlib = DeviceLibrary(lib)
    everything = explain(model, dlib, np.arange(len(lib)), weights=weights)
    count = np.zeros(model.flat.num_clusters, np.int64)
    for m in everything.match:
        count[m[m >= 0]] += 1
    top = [int(a) for a in np.argsort(-count, kind="stable")[:3]]
    con = dict(require=[[top[1], top[2]]], exclude=[top[0]])
    base = explain(model, dlib, np.arange(len(lib)), weights=weights, **con)
    assert any(not same_rows(base, r, everything, r) for r in range(len(lib))) and max(m.max() for m in base.conf_max if m.size) > 0

    def same(ex, rows):
        for r, i in enumerate(rows):
            assert same_rows(ex, r, base, i), (r, i)

    for env in ({"PMX_SLICE_KB": "8"}, {"PMX_SLICE_KB": "8", "PMX_BIG_SLICE_MB": "1", "PMX_BIG_TOTAL_MB": "64"}):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            same(explain(model, dlib, np.arange(len(lib)), weights=weights, **con), np.arange(len(lib)))
            screen(model, dlib, weights=weights, float64=True)
            assert last_score_stats()["n_slice_overflow"] > 0, env  # the setting does reach the overflow passes

    rng = np.random.default_rng(3)
    perm = rng.permutation(len(lib))
    same(explain(model, dlib, perm, weights=weights, **con), perm)
    sub = perm[:17]
    rep = np.concatenate([sub, sub[::-1], sub[:3]])
    same(explain(model, dlib, rep, weights=weights, **con), rep)
    out = {}

    def run(k):
        with torch.cuda.stream(torch.cuda.Stream()):
            out[k] = explain(model, dlib, perm, weights=weights, **con)

    ts = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    same(out[0], perm)
    same(out[1], perm)
    from pharmaconet_amd.engine import release_workspaces

    release_workspaces()  # (the two streams' workspaces hold an arena each: handed back for the large-library tests that follow)


def test_edge_cases():
    from pharmaconet_amd import PackedLibrary
    from pharmaconet_amd._ffi import PmxError
    from pharmaconet_amd.engine import explain
    from pharmaconet_amd.library import UNSUPPORTED_RECORD, LigandFeatures, pack_ligand

    model, lib, _, _ = load_golden("set_c21_c8")
    K = model.flat.num_clusters
    for bad in (dict(require=[[]]), dict(require=[[0], []]), dict(require=[[K]]), dict(exclude=[K]), dict(require=[[a] for a in range(9)])):
        with pytest.raises(PmxError):
            explain(model, lib, [0, 1], **bad)
    assert explain(model, lib, [0], require=[[a] for a in range(8)]).status.tolist() == [0]  # (8 groups are allowed)
    zero = pack_ligand(LigandFeatures([6, 8], [[1], [0]], [], np.zeros((2, 4, 3), np.float32)))
    hal = pack_ligand(LigandFeatures([6, 17], [[1], [0]], [("Halogen", 1, 1)], np.ones((2, 4, 3), np.float32)))
    small = PackedLibrary.from_records([zero, hal, UNSUPPORTED_RECORD, lib.record(0)])
    plain = explain(model, small, [3])
    a = int(plain.match[0][plain.best_conformer[0]].max())
    assert a >= 0
    # infeasible: a cluster required alone and excluded - status 0, maxima 0, no keys, best conformer 0
    for con in (dict(require=[[a]], exclude=[a]), dict(require=[[a]], exclude=list(range(K)))):
        ex = explain(model, small, [3, 3], **con)
        assert ex.status.tolist() == [0, 0] and ex.best_conformer.tolist() == [0, 0]
        for r in range(2):
            assert (ex.conf_max[r] == 0).all() and len(ex.conf_max[r]) == len(plain.conf_max[0]) and (ex.match[r] == -1).all()
            assert ex.levels[r].tolist() == plain.levels[0].tolist()
        assert ex.scores.tolist() == [0.0, 0.0]
    ex = explain(model, small, [0, 1, 2, 3, 4], require=[[a]])
    assert ex.status.tolist() == [0, 0, 1, 0, 1]  # (index 4 is outside the library)
    for r in (0, 1):
        assert (ex.conf_max[r] == 0).all() and len(ex.conf_max[r]) == 4 and ex.match[r].size == 0 and ex.best_conformer[r] == 0
    assert np.isnan(ex.conf_max[2]).all() and ex.best_conformer[2] == -1 and np.isnan(ex.scores[2]) and np.isnan(ex.scores[4])
    assert np.array_equal(ex.conf_max[3][plain.best_conformer[0]], plain.conf_max[0][plain.best_conformer[0]])
    assert explain(model, small, [], require=[[a]]).indices.size == 0
    det = model.scoring_detail(lib.record(0), exclude=[a])
    one = explain(model, small, [3], exclude=[a])
    assert np.array_equal(det["conf_max"], one.conf_max[0]) and det["score"] == float(one.scores[0]) and det["score"] < float(plain.scores[0])


def brute_force(model, lib, weights, k, require, exclude):
    from pharmaconet_amd.engine import explain

    ex = explain(model, lib, np.arange(len(lib)), weights=weights, require=require, exclude=exclude)
    cs = np.nan_to_num(ex.scores, nan=0.0)
    hits = np.flatnonzero(cs > 0)
    order = hits[np.lexsort((hits, -cs[hits]))][:k]
    return order, cs[order], ex


def test_screen_constrained():
    """set_6oim_c8 (304 ligands), k = 10, pools from 16 so that several doubling rounds run: the hits are those of a constrained explain
    of every ligand ranked on the host."""
    from pharmaconet_amd.engine import DeviceLibrary, explain, screen, screen_constrained

    model, lib, weights, _ = load_golden("set_6oim_c8")
    dlib = DeviceLibrary(lib)
    res = screen(model, dlib, weights=weights, topk=10)
    top = explain(model, dlib, [i for i, _ in res.ranking()], weights=weights)
    count = np.zeros(model.flat.num_clusters, np.int64)
    for r in range(len(top)):
        m = top.match[r][top.best_conformer[r]]
        count[m[m >= 0]] += 1
    common = int(np.argmax(count))
    sc = res.scores.cpu().numpy()
    pools, all_hits = [], {}
    for require, exclude in (([[common]], []), ([], [common])):
        want_i, want_s, _ = brute_force(model, dlib, weights, len(lib), require, exclude)  # (one walk of the whole set per constraint)
        all_hits[bool(require)] = (want_i, want_s)
        want_i, want_s = want_i[:10], want_s[:10]
        got = screen_constrained(model, dlib, 10, require=require, exclude=exclude, weights=weights, pool=16)
        assert got.exact and got.indices.tolist() == want_i.tolist() and np.array_equal(got.scores, want_s)
        assert got.scores.dtype == np.float64 and got.unconstrained.dtype == np.float32 and np.array_equal(got.unconstrained, sc[got.indices])
        assert got.explanation.indices.tolist() == want_i.tolist() and np.array_equal(got.explanation.scores, want_s)
        assert (got.scores > 0).all() and (np.diff(got.scores) <= 0).all() and (got.scores <= got.unconstrained.astype(np.float64) * (1 + 1e-6)).all()
        pools.append(got.pool)
        capped = screen_constrained(model, dlib, 10, require=require, exclude=exclude, weights=weights, pool=16, max_pool=16)
        assert capped.pool == 16 and capped.exact == (got.pool == 16)
        assert (model.screen_constrained(lib, 10, require=require, exclude=exclude, weights=weights, pool=16).indices == got.indices).all()
    assert min(pools) < len(lib)
    # fewer than k ligands satisfy it: only those come back, and the whole library was looked at
    want_i, want_s = all_hits[True]
    assert 10 < len(want_i) < len(lib)
    got = screen_constrained(model, dlib, len(want_i) + 5, require=[[common]], weights=weights, pool=16)
    assert got.exact and got.pool == len(lib) and got.indices.tolist() == want_i.tolist() and np.array_equal(got.scores, want_s)


def test_cli(tmp_path, capsys):
    from pharmaconet_amd.engine import key_qualifies
    from pharmaconet_amd.screening import main

    model, lib, weights, _ = load_golden("set_6oim_c1")
    libfile = tmp_path / "lib.pmxlib"
    lib.save(libfile)
    args = ["-p", str(GOLDEN / "model_6oim_like.pm"), "-d", str(libfile)]
    main(args + ["-o", str(tmp_path / "plain.csv")])
    ex = model.explain(lib, [int((tmp_path / "plain.csv").read_text().splitlines()[1].split(",")[0].split("#")[-1])])
    key = ex.match[0][ex.best_conformer[0]]
    a, b = int(key[key >= 0][0]), int(key[key >= 0][-1])
    other = next(c for c in range(model.flat.num_clusters) if c not in (a, b))
    main(args + ["-o", str(tmp_path / "with.csv"), "--require", f"{a},{other}", "--require", str(a), "--exclude", str(b) if b != a else str(other),
                 "--constrained_out", str(tmp_path / "con.csv"), "--constrained_k", "5"])
    assert (tmp_path / "plain.csv").read_bytes() == (tmp_path / "with.csv").read_bytes()
    rows = (tmp_path / "con.csv").read_text().splitlines()
    assert rows[0] == "rank,path,constrained_score,score,best_conformer,matches" and len(rows) == 6
    require, exclude = ((a, other), (a,)), ((b,) if b != a else (other,))
    scores = []
    for r, row in enumerate(rows[1:]):
        f = row.split(",")
        assert int(f[0]) == r + 1 and f[5]
        scores.append(float(f[2]))
        assert 0 < float(f[2]) <= float(f[3]) * (1 + 1e-6)
        matched = [int(pair.split("->")[1].split(":")[0]) for pair in f[5].split(" ")]
        assert key_qualifies(matched, require, exclude), row
    assert (np.diff(scores) <= 0).all()
    from pharmaconet_amd.screening import Screening_ArgParser

    assert Screening_ArgParser().parse_args(args + ["-o", "x.csv", "--exclude", "1", "--constrained_out", "y.csv"]).constrained_k == 100
    for misuse in (["--require", "1"], ["--exclude", "1"], ["--require", "x", "--constrained_out", str(tmp_path / "e.csv")],
                   ["--constrained_out", str(tmp_path / "e.csv"), "--constrained_k", "0"]):
        with pytest.raises(SystemExit) as err:
            main(args + ["-o", str(tmp_path / "e0.csv")] + misuse)
        assert err.value.code == 2
    capsys.readouterr()
