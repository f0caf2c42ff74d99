"""`pmx_pose_fit` on the GPU (csrc/pmx_pose_fit.hip) against the NumPy restatement of tests/pose_fit_ref.py: free mode over the record, stride
and model sizes at which the kernel's trips change (the seeded cases of `pose_fit_ref.free_case`), key mode on the golden sets' own poses
and on their second binding mode, the exact rows, rows that are not valid, repeatability, and the Python layer and the command line on top.

Bars. Integers (counts, targets, hotspot nodes, fingerprints, statuses) must be equal; they can only differ where a pair stands within
rounding of the 2-sigma threshold or two z2 within rounding of each other, so every test asserts the restatement's `margin` to be at least
1e-9 (for the seeded cases tests/test_pose_fit_cpu.py does so on the CPU as well). A z2 is a handful of correctly rounded float64
operations: 1e-12 * max(1, |value|). `node_fit`, `node_best` and `summary` are sums of non-negative terms in the restatement's own order
whose terms differ only by the two exp implementations, each within about an ulp: 1e-13 * value + 1e-300 - more than 100 times the derived
4.4e-16, and no bar for subnormal terms."""

import dataclasses
from functools import lru_cache

import numpy as np
import pytest

import pose_fit_ref as pfr
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

MARGIN = 1e-9
FIELDS = ("indices", "conformers", "fit", "ideal", "fraction", "best_fit", "best_ideal", "best_fraction", "n_nodes", "n_pairs", "n_in_place", "n_passing", "occupied_fingerprint",
          "status")
LISTS = ("node_fit", "node_best", "node_z2", "node_target", "hotspot_z2", "hotspot_node")


def same_fit(a, b, rows=None, skip=()):
    """`a` equals `b` (its rows `rows`) bit for bit."""
    rows = np.arange(len(b)) if rows is None else np.asarray(rows)
    eq = lambda x, y: np.array_equal(x, y, equal_nan=True)  # noqa: E731
    return (len(a) == len(rows) and all(eq(getattr(a, f), getattr(b, f)[rows]) for f in FIELDS if f not in skip)
            and all(eq(getattr(a, f)[k], getattr(b, f)[j]) for f in LISTS for k, j in enumerate(rows)))


def within(got, want, rel, floor):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    fin = np.isfinite(want)
    return np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]) and bool((np.abs(got[fin] - want[fin]) <= rel * np.maximum(floor, np.abs(want[fin])) + 1e-300).all())


def check_fit(pf, ref, tag, margin=True):
    """Every row of `pf` against the restatement's rows `ref`; the worst figures are printed before anything is asserted."""
    assert len(pf) == len(ref), tag
    low = min([r["margin"] for r in ref], default=np.inf)
    worst_z = worst_g = 0.0
    for i, r in enumerate(ref):
        if r["status"] != 0:
            continue
        for got, want in ((pf.node_z2[i], r["node_z2"]), (pf.hotspot_z2[i], r["hotspot_z2"])):
            fin = np.isfinite(want) & (np.asarray(got).shape == want.shape)
            if fin.any():
                worst_z = max(worst_z, float((np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))).max()))
        for got, want in ((pf.node_fit[i], r["node_fit"]), (pf.node_best[i], r["node_best"]), ([pf.fit[i], pf.ideal[i], pf.best_fit[i], pf.best_ideal[i]], r["summary"])):
            got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
            pos = want > 1e-280
            if got.shape == want.shape and pos.any():
                worst_g = max(worst_g, float((np.abs(got[pos] - want[pos]) / want[pos]).max()))
    print(f"{tag}: rows {len(ref)} margin {low:.3e} worst z2 error {worst_z:.3e} (bar 1e-12) worst fit error {worst_g:.3e} (bar 1e-13)")
    if margin:
        assert low >= MARGIN, (tag, low)
    for i, r in enumerate(ref):
        where = (tag, i)
        assert pf.status[i] == r["status"], where
        assert [int(v) for v in (pf.n_nodes[i], pf.n_pairs[i], pf.n_in_place[i], pf.n_passing[i])] == r["count"].tolist(), (where, r["count"])
        assert np.array_equal(pf.node_target[i], r["node_target"]), where
        assert np.array_equal(pf.hotspot_node[i], r["hotspot_node"]), where
        assert np.array_equal(pf.occupied_fingerprint[i], r["fingerprint"]), where
        assert within(pf.node_z2[i], r["node_z2"], 1e-12, 1.0) and within(pf.hotspot_z2[i], r["hotspot_z2"], 1e-12, 1.0), where
        assert within(pf.node_fit[i], r["node_fit"], 1e-13, 0.0) and within(pf.node_best[i], r["node_best"], 1e-13, 0.0), where
        assert within([pf.fit[i], pf.ideal[i], pf.best_fit[i], pf.best_ideal[i]], r["summary"], 1e-13, 0.0), (where, pf.fit[i], r["summary"])
        if r["status"] == 0:
            assert pf.fraction[i] == (pf.fit[i] / pf.ideal[i] if pf.ideal[i] != 0 else 0.0) and pf.best_fraction[i] == (pf.best_fit[i] / pf.best_ideal[i] if pf.best_ideal[i] != 0 else 0.0)
            assert pf.occupied(i).tolist() == [m for m in range(256) if (int(r["fingerprint"][m // 64]) >> (m % 64)) & 1], where


def run_free(c, rows=None, **kw):
    from pharmaconet_amd.engine import pose_fit

    rows = np.arange(len(c["indices"])) if rows is None else np.asarray(rows, dtype=np.int64)
    over = dict(centers=c["centers"], sigmas=c["sigmas"]) if c["override"] else {}
    over.update(kw)
    return pose_fit(c["model"], c["lib"], c["indices"][rows], c["conformers"][rows], c["rotation"][rows], c["translation"][rows], weights=c["weights"], **over)


@lru_cache(maxsize=None)
def free_result(nm, stride):
    return run_free(pfr.free_case(nm, stride))


# ---------------------------------------------------------------------------------------------------------------- 1. free mode
@pytest.mark.parametrize("nm,stride", pfr.FREE_CASES)
def test_free_mode_against_the_restatement(nm, stride):
    c = pfr.free_case(nm, stride)
    pf = free_result(nm, stride)
    check_fit(pf, c["ref"], f"free, {nm} model nodes, stride {stride}")
    assert {1, 2, 63, 64} <= {len(x) for x in pf.node_fit} and all(len(x) == nm for x in pf.hotspot_z2)
    assert (pf.n_passing > 0).any() and pf.occupied_fingerprint.any()
    if nm > 192:
        assert pf.occupied_fingerprint[:, 3].any() and any((x[192:] >= 0).any() for x in pf.hotspot_node)
    if nm == 37:  # the model's own centres and radii are the default
        assert same_fit(run_free(c, centers=c["model"].node_centers, sigmas=c["model"].node_radii), pf)


def test_calls_of_no_row_and_one_row():
    from pharmaconet_amd.engine import pose_fit

    c = pfr.free_case(37, 1)
    full = free_result(37, 1)
    none = run_free(c, rows=[])
    assert len(none) == 0 and none.occupied_fingerprint.shape == (0, 4) and none.fit.shape == (0,) and none.node_fit == []
    for r in (0, 5, 96):
        assert same_fit(run_free(c, rows=[r]), full, rows=[r])
    with pytest.raises(ValueError):
        run_free(c, centers=c["centers"][:-1])
    with pytest.raises(ValueError):
        run_free(c, sigmas=np.ones(38))
    with pytest.raises(ValueError):
        pose_fit(c["model"], c["lib"], [0, 1], [0], np.zeros((2, 3, 3)), np.zeros((2, 3)))


# ---------------------------------------------------------------------------------------------------------------- 2. key mode
@lru_cache(maxsize=None)
def explained(name):
    """A set's first hits with small trees, explained with two modes, and the fit of mode 0 and of mode 1: computed once, never written to."""
    from pharmaconet_amd.engine import explain_modes
    from test_gpu_pose_search import small_trees

    model, lib, weights, d = load_golden(name)
    idx = small_trees(d, 4 if "l110" in name else 12)
    ms = explain_modes(model, lib, idx, modes=2, weights=weights)
    return model, lib, weights, ms


def key_reference(model, lib, weights, ex, al, keys):
    from pharmaconet_amd.constants import weights_vector

    w7 = weights_vector(weights)
    types, Y, S = np.asarray(model.flat.node_type), model.node_centers, model.node_radii
    ref = []
    for r in range(len(al)):
        rec = lib.unpack(int(al.indices[r]))
        c = int(al.conformers[r])
        pairs = pfr.key_pairs(model, rec, w7, ex.levels[int(al.rows[r])], keys[r], c)
        ref.append(pfr.fit_row(types, Y, S, w7, rec, c, al.rotation[r], al.translation[r], pairs))
    return ref


@pytest.mark.parametrize("name", ["set_6oim_c8", "set_c21_c8", "set_l110_c8", "set_s64_c8"])
def test_key_mode_on_the_sets_own_poses_and_on_their_second_mode(name):
    from pharmaconet_amd.engine import pose_fit

    model, lib, weights, ms = explained(name)
    fitted = 0
    for mode in (0, 1):
        ex = ms.explanation(mode)
        rows, conf, keys = ex._own_rows(None)
        al = ex.poses(model, lib, weights=weights)
        pf = al.pose_fit(model, lib, keys=keys, weights=weights)
        check_fit(pf, key_reference(model, lib, weights, ex, al, keys), f"key, {name}, mode {mode}")
        ok = al.status == 0
        assert np.array_equal(pf.status == 0, ok) and np.array_equal(pf.n_nodes[ok], al.n_nodes[ok]) and np.array_equal(pf.n_pairs[ok], al.n_pairs[ok])
        fitted += int((pf.n_pairs > 0).sum())
        # `Explanation.pose_fit` fits as `poses` does and scores under the same key; free mode sees at least these pairs
        assert same_fit(ex.pose_fit(model, lib, weights=weights), pf)
        free = al.pose_fit(model, lib, weights=weights)
        assert (free.n_pairs >= pf.n_pairs).all() and (free.n_passing >= pf.n_passing).all()
        assert same_fit(pose_fit(model, lib, al.indices, al.conformers, al.rotation, al.translation, keys=keys, weights=weights), pf)
    assert fitted >= 4


# ---------------------------------------------------------------------------------------------------------------- 3. exact rows
def test_exact_rows_on_the_centre_and_at_two_sigma():
    """One model node left with a sigma (the others NaN), at a centre that is exact in float32: a ligand node of its type on the centre has
    z2 = 0, g = w and fraction exactly 1.0; at an offset of (2, 0, 0) with sigma 1, d2 = 4 = 4 v and the pair does not pass; one float32
    step closer it does. The rows of tests/test_pose_fit_cpu.py, bit for bit."""
    from ligand_fp_ref import make_record
    from pharmaconet_amd import PackedLibrary
    from pharmaconet_amd.constants import weights_vector
    from pharmaconet_amd.engine import pose_fit

    model, _, weights, _ = load_golden("set_6oim_c8")
    nm, a = model.num_nodes, 5
    ty = int(model.flat.node_type[a])
    w = float(np.float32(weights_vector(weights)[ty]))
    centers, sigmas = model.node_centers.copy(), np.full(nm, np.nan)
    centers[a], sigmas[a] = (3.0, -2.0, 5.0), 1.0
    inside = float(np.nextafter(np.float32(5.0), np.float32(0)))
    pts = [(3.0, -2.0, 5.0), (5.0, -2.0, 5.0), (inside, -2.0, 5.0)]
    lib = PackedLibrary.from_records([make_record([1 << ty], np.array(p, np.float32).reshape(1, 1, 3)) for p in pts])
    eye, zero = np.eye(3), np.zeros(3)
    pf = pose_fit(model, lib, [0, 1, 2], [0, 0, 0], [eye] * 3, [zero] * 3, weights=weights, centers=centers, sigmas=sigmas)
    ref = [pfr.fit_row(model.flat.node_type, centers, sigmas, weights_vector(weights), lib.unpack(i), 0, eye, zero) for i in range(3)]
    assert pf.status.tolist() == [0, 0, 0] and pf.n_nodes.tolist() == [1, 1, 1] and pf.n_pairs.tolist() == [1, 1, 1]
    assert pf.n_passing.tolist() == [1, 0, 1] and pf.n_in_place.tolist() == [1, 0, 1]
    assert pf.node_z2[0][0] == 0.0 and pf.fit[0] == w and pf.ideal[0] == w and pf.fraction[0] == 1.0 and pf.best_fraction[0] == 1.0
    assert pf.node_z2[1][0] == 4.0 and pf.occupied(1).tolist() == [] and pf.occupied(0).tolist() == [a] and pf.occupied(2).tolist() == [a]
    assert pf.node_z2[2][0] == (inside - 3.0) ** 2 < 4.0
    for i, r in enumerate(ref):
        got = [pf.fit[i], pf.ideal[i], pf.best_fit[i], pf.best_ideal[i]]
        print(f"exact row {i}: fit {pf.fit[i]!r} restatement {r['summary'][0]!r}")
        assert np.array_equal(got, r["summary"]) and np.array_equal(pf.node_fit[i], r["node_fit"]) and np.array_equal(pf.node_z2[i], r["node_z2"]), i
        assert np.array_equal(pf.hotspot_z2[i], r["hotspot_z2"]) and np.array_equal(pf.hotspot_node[i], r["hotspot_node"]) and np.array_equal(pf.node_target[i], r["node_target"]), i
        assert np.array_equal(pf.occupied_fingerprint[i], r["fingerprint"]), i


# ---------------------------------------------------------------------------------------------------------------- 4. rows that are not valid
def assert_not_ok(pf, i, n_nodes, nm):
    assert np.isnan([pf.fit[i], pf.ideal[i], pf.best_fit[i], pf.best_ideal[i]]).all() and (pf.n_nodes[i], pf.n_pairs[i], pf.n_in_place[i], pf.n_passing[i]) == (0, 0, 0, 0)
    assert not pf.occupied_fingerprint[i].any() and len(pf.node_fit[i]) == n_nodes and len(pf.hotspot_z2[i]) == nm
    assert np.isnan(pf.node_fit[i]).all() and np.isnan(pf.node_best[i]).all() and np.isnan(pf.node_z2[i]).all() and (pf.node_target[i] == -1).all()
    assert np.isnan(pf.hotspot_z2[i]).all() and (pf.hotspot_node[i] == -1).all()


def test_rows_that_are_not_valid_pass_through_and_leave_their_neighbours_alone():
    from explain_ref import candidates
    from pharmaconet_amd.engine import pose_fit

    c = pfr.free_case(37, 1)
    full = free_result(37, 1)
    model, lib = c["model"], c["lib"]
    good = [0, 1, 2, 3, 4, 5, 6]
    idx, conf, rot, trans = c["indices"][good].copy(), c["conformers"][good].copy(), c["rotation"][good].copy(), c["translation"][good].copy()
    idx[0] = len(lib)
    conf[2], conf[3] = -1, 1  # (the case's records have one conformer)
    rot[5][1, 2] = np.nan
    pf = pose_fit(model, lib, idx, conf, rot, trans, weights=c["weights"])
    assert pf.status.tolist() == [1, 0, 4, 4, 0, 4, 0]
    for i in (0, 2, 3, 5):
        assert_not_ok(pf, i, 0 if i == 0 else int(lib.header(int(idx[i]))[0]), 37)
    keep = [1, 4, 6]
    sub = dataclasses.replace(pf, **{f: getattr(pf, f)[keep] for f in FIELDS}, **{f: [getattr(pf, f)[k] for k in keep] for f in LISTS})
    assert same_fit(sub, full, rows=keep)
    # a sigma of 0 or NaN takes one model node out and leaves every other pair as it was; a weight of 0 takes a type out
    for bad in (0.0, np.nan):
        s = c["sigmas"].copy()
        s[3] = bad
        got = run_free(c, sigmas=s)
        ref = [pfr.fit_row(c["node_type"], c["centers"], s, c["w7"], lib.unpack(int(i)), int(cc), c["rotation"][r], c["translation"][r])
               for r, (i, cc) in enumerate(zip(c["indices"], c["conformers"]))]
        check_fit(got, ref, f"sigma[3] = {bad}")
        assert all(np.isinf(x[3]) and h[3] == -1 for x, h in zip(got.hotspot_z2, got.hotspot_node)) and not (got.occupied_fingerprint[:, 0] >> np.uint64(3) & np.uint64(1)).any()
        other = [m for m in range(37) if m != 3]
        assert all(np.array_equal(x[other], y[other]) for x, y in zip(got.hotspot_z2, full.hotspot_z2))
    from pharmaconet_amd.constants import TYPE_NAMES, weights_vector

    ty = int(c["node_type"][0])
    w7 = np.array(weights_vector(c["weights"]), dtype=np.float32)
    w7[ty] = 0.0
    w0 = {TYPE_NAMES[t]: float(w7[t]) for t in range(7)}
    assert np.array_equal(np.asarray(weights_vector(w0), dtype=np.float32), w7)
    got = pose_fit(model, lib, c["indices"], c["conformers"], c["rotation"], c["translation"], weights=w0)
    ref = [pfr.fit_row(c["node_type"], c["centers"], c["sigmas"], w7, lib.unpack(int(i)), int(cc), c["rotation"][r], c["translation"][r])
           for r, (i, cc) in enumerate(zip(c["indices"], c["conformers"]))]
    check_fit(got, ref, f"weight of type {ty} = 0")
    assert all((h[c["node_type"] == ty] == -1).all() for h in got.hotspot_node) and (got.n_pairs < full.n_pairs).any()
    # key mode: a match that is no candidate of its level
    model, lib, weights, ms = explained("set_6oim_c8")
    ex = ms.explanation(0)
    rows, conf, keys = ex._own_rows(None)
    al = ex.poses(model, lib, weights=weights)
    r = next(r for r in range(len(al)) if al.n_pairs[r] > 0 and len(ex.levels[rows[r]]) > 0)
    rec = lib.unpack(int(al.indices[r]))
    wrong = next(a for a in range(model.flat.num_clusters) if a not in candidates(model, rec, int(ex.levels[rows[r]][0])))
    bad_keys = [np.array(k).copy() for k in keys]
    bad_keys[r][0] = wrong
    good_pf = al.pose_fit(model, lib, keys=keys, weights=weights)
    bad_pf = al.pose_fit(model, lib, keys=bad_keys, weights=weights)
    assert bad_pf.status[r] == 4 and good_pf.status[r] == 0
    assert_not_ok(bad_pf, r, int(rec["n_nodes"]), model.num_nodes)
    others = [k for k in range(len(al)) if k != r]
    sub = dataclasses.replace(bad_pf, **{f: getattr(bad_pf, f)[others] for f in FIELDS}, **{f: [getattr(bad_pf, f)[k] for k in others] for f in LISTS})
    assert same_fit(sub, good_pf, rows=others)


# ---------------------------------------------------------------------------------------------------------------- 5. repeatability
def test_same_bits_twice_and_under_a_permutation_of_the_rows():
    c = pfr.free_case(222, 64)
    a = free_result(222, 64)
    assert same_fit(run_free(c), a)
    perm = np.random.default_rng(3).permutation(len(a))
    assert same_fit(run_free(c, rows=perm), a, rows=perm)
    model, lib, weights, ms = explained("set_6oim_c8")
    ex = ms.explanation(0)
    _, _, keys = ex._own_rows(None)
    al = ex.poses(model, lib, weights=weights)
    k = al.pose_fit(model, lib, keys=keys, weights=weights)
    perm = np.random.default_rng(4).permutation(len(al))
    from pharmaconet_amd.engine import pose_fit

    again = pose_fit(model, lib, al.indices[perm], al.conformers[perm], al.rotation[perm], al.translation[perm], keys=[keys[j] for j in perm], weights=weights)
    assert same_fit(again, k, rows=perm)


# ---------------------------------------------------------------------------------------------------------------- 6. the layer above
def test_refined_poses_pose_search_and_scoring_pose_fit():
    from pharmaconet_amd.engine import pose_fit
    from test_gpu_clash import pocket_6oim

    model, lib, weights, ms = explained("set_6oim_c8")
    pocket = pocket_6oim()
    ex = ms.explanation(0)
    rows, conf, keys = ex._own_rows(None)
    al = ex.poses(model, lib, weights=weights)
    before = al.pose_fit(model, lib, keys=keys, weights=weights)
    ref = al.refine(pocket, lib)
    after = ref.pose_fit(model, lib, keys=keys, weights=weights)
    assert same_fit(after, pose_fit(model, lib, ref.indices, ref.conformers, ref.rotation, ref.translation, keys=keys, weights=weights))
    still = np.flatnonzero(ref.stop == 0)
    moved = np.flatnonzero(ref.accepted > 0)
    print(f"refine: {len(still)} rows untouched, {len(moved)} moved; fraction before {before.fraction[moved]} after {after.fraction[moved]}")
    assert len(still) > 0 and len(moved) > 0
    pick = lambda pf, rr: dataclasses.replace(pf, **{f: getattr(pf, f)[rr] for f in FIELDS}, **{f: [getattr(pf, f)[k] for k in rr] for f in LISTS})  # noqa: E731
    assert same_fit(pick(after, still), before, rows=still)  # (a row the refinement left untouched has the fit it had, bit for bit)
    assert not same_fit(pick(after, moved), before, rows=moved)
    # the search's chosen rows under the chosen keys
    ps = ms.pose_search(model, lib, pocket, weights=weights)
    chosen = ps.pose_fit(model, lib, weights=weights)
    pa = ps.alignment()
    assert same_fit(chosen, pose_fit(model, lib, pa.indices, pa.conformers, pa.rotation, pa.translation, keys=ps.key, weights=weights))
    assert np.array_equal(chosen.status == 0, ps.conformer >= 0) and np.array_equal(chosen.n_pairs[chosen.status == 0], pa.n_pairs[chosen.status == 0])
    # similarity and leaders go through the fingerprint calls
    from pharmaconet_amd.engine import fingerprint_similarity

    assert np.array_equal(before.similarity(), fingerprint_similarity(before.occupied_fingerprint)) and before.similarity(after).shape == (len(before), len(after))
    leaders, leader_of = before.leaders(threshold=0.5)
    assert leaders[0] == 0 and len(leader_of) == len(before)
    r = int(np.argmax(before.n_pairs))
    from pharmaconet_amd.constants import weights_vector

    positive = int(np.count_nonzero(np.asarray(weights_vector(weights))[np.asarray(model.flat.node_type)] > 0))
    assert before.coverage(r, model, weights) == len(before.occupied(r)) / positive
    # one ligand
    one = model.scoring_pose_fit(lib.record(int(al.indices[r])), weights=weights, refine=True, pocket=pocket)
    assert one["conformer"] == al.conformers[r] and one["fit"] == before.fit[r] and one["fraction"] == before.fraction[r] and one["n_pairs"] == before.n_pairs[r]
    assert np.array_equal(one["occupied"], before.occupied(r)) and one["refined"]["fit"] == after.fit[r] and one["refined"]["stop"] == ref.stop[r]
    assert "refined" not in model.scoring_pose_fit(lib.record(int(al.indices[r])), weights=weights)


def test_fitting_with_fit_keeps_every_field_it_had():
    from test_gpu_clash import pocket_6oim

    from test_gpu_pose_search import small_trees

    model, lib, weights, d = load_golden("set_6oim_c8")
    pocket = pocket_6oim()
    lib = lib.select(small_trees(d, 12))  # (ligands whose trees are walked in milliseconds: the screen is not what is tested)
    res = model.screen(lib, weights=weights)
    for kw in (dict(), dict(refine=True, refine_tolerance=0.0)):
        plain = res.fitting(12, pool=12, pocket=pocket, **kw)
        fit = res.fitting(12, pool=12, pocket=pocket, fit=True, **kw)
        assert plain.fit is None and fit.fit is not None and len(fit.fit) == len(fit.poses)
        for f in dataclasses.fields(plain):
            a, b = getattr(plain, f.name), getattr(fit, f.name)
            if f.name == "fit":
                continue
            if dataclasses.is_dataclass(a):
                for g in dataclasses.fields(a):
                    x, y = getattr(a, g.name), getattr(b, g.name)
                    assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(x, y)) and len(x) == len(y) if isinstance(x, list) else np.array_equal(x, y, equal_nan=True), (f.name, g.name)
            else:
                assert (a is None and b is None) or np.array_equal(a, b, equal_nan=True), f.name
        al = fit.poses
        assert same_fit(fit.fit, al.pose_fit(model, lib, weights=weights))  # (at the motion finally used, free mode)


def test_cli_pose_fit_csv(tmp_path):
    from pharmaconet_amd.screening import POSE_FIT_HEADER, main

    from test_gpu_pose_search import small_trees

    model, lib, _, d = load_golden("set_6oim_c8")
    lib = lib.select(small_trees(d, 8))  # (a screen of 8 ligands with small trees: the command line is what is tested)
    libfile = tmp_path / "lib.pmxlib"
    lib.save(libfile)
    args = ["-p", str(GOLDEN / "model_6oim_like.pm"), "-d", str(libfile), "--explain", "5", "--protein", str(GOLDEN / "pocket_6oim.pdb"), "--clash_level", "nodes"]
    main(args + ["-o", str(tmp_path / "plain.csv"), "--explain_out", str(tmp_path / "plain_hits.csv"), "--refine_out", str(tmp_path / "plain_refine.csv")])
    main(args + ["-o", str(tmp_path / "with.csv"), "--explain_out", str(tmp_path / "hits.csv"), "--refine_out", str(tmp_path / "refine.csv"), "--pose_fit", str(tmp_path / "fit.csv"),
                 "--pose_fit_mode", "free"])
    for a, b in (("plain.csv", "with.csv"), ("plain_hits.csv", "hits.csv"), ("plain_refine.csv", "refine.csv")):
        assert (tmp_path / a).read_bytes() == (tmp_path / b).read_bytes()
    hits = (tmp_path / "hits.csv").read_text().splitlines()[1:]
    rows = (tmp_path / "fit.csv").read_text().splitlines()
    assert POSE_FIT_HEADER == "rank,path,conformer,stage,fitted_nodes,pairs,in_place,passing,fit,ideal,fraction,best_fit,best_fraction,occupied_nodes"
    assert rows[0] == POSE_FIT_HEADER and len(rows) == 2 * len(hits) + 1 == 11
    assert [r.split(",")[3] for r in rows[1:]] == ["fit", "refined"] * 5 and all(len(r.split(",")) == 14 for r in rows[1:])
    with pytest.raises(SystemExit):
        main(["-p", str(GOLDEN / "model_6oim_like.pm"), "-d", str(libfile), "-o", str(tmp_path / "x.csv"), "--pose_fit", str(tmp_path / "f.csv")])  # no --explain
