"""`pmx_align` on the GPU (csrc/pmx_rows.hip): the rigid fit of listed (ligand, conformer, key) rows against the NumPy restatement of
tests/align_ref.py (an SVD fit, where the kernel diagonalises Horn's matrix), a planted pose and its mirror image, degenerate and invalid
rows, repeatability, and the Python layer on top of it.

Bars. Every sum on either side is a float64 sum of fewer than 10^4 terms of at most E0 each, so two sides differ by at most about
10^4 * 1.1e-16 * E0; the bar is 1e-10 * E0. Where E0 itself is rounding noise (one fitted node with one target: every difference the sums
are made of is zero but for the rounding of coordinates of size A), the same reasoning gives W * (16 * eps * A)^2, which is added: `bar()`.
A rotation is compared only where it is unique, gap >= 1e-4 * E0 (the restatement's gap): its error is about eps * E0 / gap <= 1e-11 rad,
on arms below 100 A that is 1e-9 A, and the bar on posed positions is 1e-8 A."""

from functools import lru_cache

import numpy as np
import pytest

import align_ref
from conftest import GOLDEN, load_golden
from explain_ref import NONE, Tables, candidates, ligand_levels
from test_gpu_attribution import SETS

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
GATE = 1e-4


def bar(ref, A):
    return 1e-10 * ref["E0"] + ref["W"] * (16 * EPS * A) ** 2


def proper(R, tol=1e-12):
    return np.abs(R @ R.T - np.eye(3)).max() <= tol and abs(np.linalg.det(R) - 1.0) <= tol


@lru_cache(maxsize=None)
def posed(name):
    """A set, the explanation of its first 32 ligands (4 of the 110-node model; with the first 64-node ligand of set_s64_c8) and the fit of
    every OK one at its best conformer under its own key: computed once, shared, never written to."""
    from pharmaconet_amd.engine import explain

    model, lib, weights, _ = load_golden(name)
    idx = list(range(min(4 if "l110" in name else 32, len(lib))))
    if name == "set_s64_c8":
        full = int(np.flatnonzero(lib.headers()[:, 0] == 64)[0])
        idx += [full] if full not in idx else []
    ex = explain(model, lib, idx, weights=weights)
    al = ex.poses(model, lib, weights=weights)
    return model, lib, weights, ex, al


def same_bits(a, b):
    eq = lambda x, y: np.array_equal(x, y, equal_nan=True)  # noqa: E731
    return (all(eq(getattr(a, f), getattr(b, f)) for f in ("rotation", "translation", "rmsd", "rmsd_nodes", "weight", "sse", "scale", "gap", "n_nodes", "n_pairs", "status"))
            and all(eq(x, y) for x, y in zip(a.node, b.node)) and all(eq(x, y) for x, y in zip(a.levels, b.levels)) and len(a) == len(b))


def check_row(al, r, ref, A, tag):
    """Row r of `al` against the restatement's `ref` (check 1 of the feature's specification); returns the deviations as fractions of the bars."""
    assert ref["valid"] and al.status[r] == 0, tag
    assert (int(al.n_nodes[r]), int(al.n_pairs[r])) == (ref["n_nodes"], ref["n_pairs"]), tag
    assert abs(al.weight[r] - ref["W"]) <= 1e-12 * ref["W"], (tag, al.weight[r], ref["W"])
    assert abs(al.scale[r] - ref["E0"]) <= 1e-12 * ref["E0"] + ref["W"] * (16 * EPS * A) ** 2, (tag, al.scale[r], ref["E0"])
    b = bar(ref, A)
    d_sse, d_rn = abs(al.sse[r] - ref["sse"]), abs(al.rmsd_nodes[r] ** 2 * al.weight[r] - ref["rn"])
    assert d_sse <= b, (tag, al.sse[r], ref["sse"], ref["E0"])
    assert d_rn <= b, (tag, al.rmsd_nodes[r] ** 2 * al.weight[r], ref["rn"], ref["E0"])
    assert proper(al.rotation[r]), (tag, al.rotation[r])
    assert abs(al.rmsd[r] - (np.sqrt(al.sse[r] / al.weight[r]) if ref["n_pairs"] else 0.0)) <= 1e-15 * max(al.rmsd[r], 1.0)
    assert np.array_equal(al.node[r] < 0, ref["node"] < 0) and (al.node[r][ref["node"] < 0] == -1.0).all(), tag
    return d_sse / b if b else 0.0, d_rn / b if b else 0.0


@pytest.mark.parametrize("name", SETS)
def test_against_the_restatement(name):
    from pharmaconet_amd.constants import weights_vector

    model, lib, weights, ex, al = posed(name)
    w7 = weights_vector(weights)
    Y = align_ref.node_centers(model)
    assert len(al) == int((ex.status == 0).sum()) > 0
    worst = np.zeros(4)
    gated = 0
    for r, i in enumerate(al.rows):
        lig, c = int(ex.indices[i]), int(ex.best_conformer[i])
        assert al.indices[r] == lig and al.conformers[r] == c and al.levels[r].tolist() == ex.levels[i].tolist()
        rec = lib.unpack(lig)
        T = Tables(model, rec, w7)
        ref = align_ref.align(model, rec, w7, ex.levels[i], ex.match[i][c], c, T, "svd", Y)
        A = max(float(np.abs(Y).max()), float(np.abs(T.pos[:, c]).max()))
        assert A < 100.0
        ds, dn = check_row(al, r, ref, A, (name, lig, c))
        worst[:2] = np.maximum(worst[:2], (ds, dn))
        if ref["n_pairs"] and ref["gap"] >= GATE * ref["E0"]:
            gated += 1
            for u, p in ref["posed"].items():
                dp = float(np.abs(al.transform(r, T.pos[u, c].astype(np.float64)) - p).max())
                dd = abs(al.node[r][u] - ref["node"][u])
                worst[2:] = np.maximum(worst[2:], (dp, dd))
                assert dp <= 1e-8 and dd <= 1e-8, (name, lig, c, u, dp, dd, ref["gap"] / ref["E0"])
    share = gated / len(al)
    print(f"{name}: {len(al)} rows; of the bar: sse {worst[0]:.3g} rmsd_nodes^2 W {worst[1]:.3g}; gated {100 * share:.0f} %: posed nodes {worst[2]:.3g} A, node deviations {worst[3]:.3g} A")
    assert share >= 0.75, (name, gated, len(al))
    if name == "set_s64_c8":
        assert max(len(x) for x in al.node) == 64  # every lane owns a node


# ---------------------------------------------------------------------------------------------------------------- a planted pose
PLANTED = ((1, "Cation"), (2, "HBond_acceptor"), (4, "HBond_acceptor"), (7, "HBond_acceptor"), (9, "Hydrophobic"), (13, "Hydrophobic"), (14, "Hydrophobic"))


def quat_rotation(q):
    q0, q1, q2, q3 = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
                     [2 * (q1 * q2 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * (q2 * q3 - q0 * q1)],
                     [2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3]])


def planted_ligand(model, mirrored: bool):
    """One single-node ligand cluster per PLANTED (model cluster, type), the node at the centroid of the cluster's nodes of that type (equal
    weights: its target centroid), taken out of the pocket by the inverse of a known motion (R0, t0) and rounded to float32; mirrored: the
    points reflected through a plane through their centroid first. Returns the one-ligand library, its levels, the key that matches every
    planted cluster, R0 and t0."""
    from pharmaconet_amd import PackedLibrary
    from pharmaconet_amd.constants import TYPE_ID
    from pharmaconet_amd.library import LigandFeatures, pack_ligand
    from pharmaconet_amd.pharmacophore_model import cluster_node_sets

    flat, Y = model.flat, align_ref.node_centers(model)
    sets = cluster_node_sets(flat)
    pts = np.array([Y[[m for m in range(flat.num_nodes) if sets[a] >> m & 1 and flat.node_type[m] == TYPE_ID[t]]].mean(axis=0) for a, t in PLANTED])
    assert np.linalg.svd(pts - pts.mean(0), compute_uv=False)[2] > 1.0  # (not coplanar)
    if mirrored:
        pts = pts * np.array([1.0, 1.0, -1.0]) + np.array([0.0, 0.0, 2.0 * pts[:, 2].mean()])
    R0, t0 = quat_rotation([0.3, -0.5, 0.7, 0.4]), np.array([7.0, -3.0, 4.5])
    x = ((pts - t0) @ R0).astype(np.float32)  # R0^T (y - t0)
    assert np.abs(x).max() < 64.0 and np.abs(Y).max() < 64.0
    k = len(PLANTED)
    lig = LigandFeatures([6] * k, [[] for _ in range(k)], [(t, j, j) for j, (_, t) in enumerate(PLANTED)], x[:, None, :])
    lib = PackedLibrary.from_records([pack_ligand(lig)])
    rec = lib.unpack(0)
    assert rec["n_nodes"] == rec["n_clusters"] == k
    levels = ligand_levels(model, rec)
    assert len(levels) == k
    key = []
    for q in levels:  # (the record orders clusters by priority: find the planted point behind each)
        j = int(np.flatnonzero((x == rec["xyz"][q, :, 0]).all(axis=1))[0])
        assert PLANTED[j][0] in candidates(model, rec, q)
        key.append(PLANTED[j][0])
    return lib, rec, levels, key, R0, t0


def test_planted_pose_and_its_mirror_image():
    """float32 rounding of coordinates below 64 A moves a point by less than 7e-6 A, so the best fit of the planted points is within that of
    every target centroid: the bars of 5e-5 A leave room for nothing else."""
    from pharmaconet_amd.constants import weights_vector
    from pharmaconet_amd.engine import align

    model, _, weights, _ = load_golden("set_c21_c8")
    w7 = weights_vector(weights)
    lib, rec, levels, key, R0, t0 = planted_ligand(model, mirrored=False)
    ref = align_ref.align(model, rec, w7, levels, key, 0)
    assert ref["n_nodes"] == len(PLANTED) and ref["n_pairs"] == len(PLANTED) + 1 and ref["spread"] > 0  # (cluster 13 holds two hydrophobic nodes)
    al = align(model, lib, [0], [0], [key], weights=weights)
    assert al.status[0] == 0 and (int(al.n_nodes[0]), int(al.n_pairs[0])) == (ref["n_nodes"], ref["n_pairs"])
    print(f"planted: sse - spread {al.sse[0] - ref['spread']:.3g} (bar {al.weight[0] * 5e-5 ** 2:.3g}), worst node {al.node[0].max():.3g} A, "
          f"|R - R0| {np.abs(al.rotation[0] - R0).max():.3g}, |t - t0| {np.abs(al.translation[0] - t0).max():.3g}")
    assert al.sse[0] - ref["spread"] <= al.weight[0] * 5e-5 ** 2
    T = Tables(model, rec, w7)
    for u, target in ref["target"].items():
        assert np.linalg.norm(al.transform(0, T.pos[u, 0].astype(np.float64)) - target) <= 5e-5
    assert proper(al.rotation[0]) and (al.node[0] <= 5e-5).all()
    assert np.abs(al.rotation[0] - R0).max() <= 1e-4 and np.abs(al.translation[0] - t0).max() <= 1e-3  # (arms of 5 A and more, positions below 20 A)

    mlib, mrec, mlevels, mkey, _, _ = planted_ligand(model, mirrored=True)
    mref = align_ref.align(model, mrec, w7, mlevels, mkey, 0)
    assert abs(np.linalg.det(mref["R"]) - 1.0) <= 1e-12 and mref["rmsd_nodes"] > 0.1 and mref["gap"] >= GATE * mref["E0"]
    ml = align(model, mlib, [0], [0], [mkey], weights=weights)
    assert ml.status[0] == 0 and abs(np.linalg.det(ml.rotation[0]) - 1.0) <= 1e-12 and ml.rmsd_nodes[0] > 0.1
    check_row(ml, 0, mref, 64.0, "mirrored")


# ---------------------------------------------------------------------------------------------------------------- degenerate and invalid rows
def test_degenerate_and_invalid_rows_in_one_call():
    from pharmaconet_amd.constants import weights_vector
    from pharmaconet_amd.engine import align

    model, lib, weights, ex, base = posed("set_6oim_c8")
    w7 = weights_vector(weights)
    Y = align_ref.node_centers(model)
    K = model.flat.num_clusters
    # a ligand with two levels or more, and for it: keys that fit exactly one node, and exactly two
    one = two = None
    for i in range(len(ex)):
        if ex.status[i] != 0 or len(ex.levels[i]) < 2:
            continue
        rec = lib.unpack(int(ex.indices[i]))
        T = Tables(model, rec, w7)
        nl = len(ex.levels[i])
        single = []
        for l in range(nl):
            for a in candidates(model, rec, int(ex.levels[i][l])):
                k = np.full(nl, NONE, dtype=np.int64)
                k[l] = a
                if align_ref.align(model, rec, w7, ex.levels[i], k, 0, T, "svd", Y)["n_nodes"] == 1:
                    single.append(k)
                    break
        if len(single) >= 2 and np.flatnonzero(single[0] >= 0)[0] != np.flatnonzero(single[1] >= 0)[0]:
            one, two, i0 = single[0], np.maximum(single[0], single[1]), i
            break
    assert one is not None
    lig = int(ex.indices[i0])
    rec0 = lib.unpack(lig)
    T0 = Tables(model, rec0, w7)
    nl, C0 = len(ex.levels[i0]), len(ex.conf_max[i0])
    none = np.full(nl, NONE, dtype=np.int64)
    stranger = one.copy()
    l0 = int(np.flatnonzero(one >= 0)[0])
    stranger[l0] = next(m for m in range(K) if m not in candidates(model, rec0, int(ex.levels[i0][l0])))
    rows = [(lig, 0, none), (lig, 0, one), (lig, 0, two), (lig, C0, one), (lig, 0, stranger), (len(lib), 0, none)]
    al = align(model, lib, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], weights=weights)
    assert al.status.tolist() == [0, 0, 0, 4, 4, 1]
    A = max(float(np.abs(Y).max()), float(np.abs(T0.pos[:, 0]).max()))
    # all-None key
    assert np.array_equal(al.rotation[0], np.eye(3)) and (al.translation[0] == 0).all()
    assert [al.weight[0], al.sse[0], al.rmsd[0], al.rmsd_nodes[0], al.scale[0], al.gap[0], al.n_nodes[0], al.n_pairs[0]] == [0] * 8
    assert len(al.node[0]) == rec0["n_nodes"] and (al.node[0] == -1.0).all()
    # one fitted node
    ref1 = align_ref.align(model, rec0, w7, ex.levels[i0], one, 0, T0, "svd", Y)
    assert np.array_equal(al.rotation[1], np.eye(3)) and al.n_nodes[1] == 1 and al.n_pairs[1] == ref1["n_pairs"]
    u = int(np.flatnonzero(ref1["node"] >= 0)[0])
    assert np.abs(al.translation[1] - ref1["t"]).max() <= 16 * EPS * A
    assert abs(al.node[1][u] - ref1["node"][u]) <= 16 * EPS * A and (np.delete(al.node[1], u) == -1.0).all()
    check_row(al, 1, ref1, A, "one node")
    # two fitted nodes
    ref2 = align_ref.align(model, rec0, w7, ex.levels[i0], two, 0, T0, "svd", Y)
    assert ref2["n_nodes"] == 2 and np.isfinite(al.rotation[2]).all() and np.isfinite(al.translation[2]).all() and np.isfinite(al.node[2]).all()
    check_row(al, 2, ref2, A, "two nodes")
    # not OK: NaN throughout, counts of zero
    for r in (3, 4, 5):
        assert np.isnan(al.rotation[r]).all() and np.isnan(al.translation[r]).all() and np.isnan(al.node[r]).all()
        assert all(np.isnan(getattr(al, f)[r]) for f in ("weight", "sse", "rmsd", "rmsd_nodes", "scale", "gap"))
        assert al.n_nodes[r] == 0 and al.n_pairs[r] == 0
    assert len(al.node[3]) == rec0["n_nodes"] and len(al.node[5]) == 0 and len(al.levels[5]) == 0
    assert al.levels[4].tolist() == ex.levels[i0].tolist()


def test_row_calls_agree_on_what_a_row_is():
    """`pmx_attribute` and `pmx_align` open a row with one front end (open_row in csrc/pmx_rows.hip) and `pmx_explain` finds the levels by the
    same rule (pmx_screen_tables.h): the same rows, good and bad, through both calls give the same status, levels and node count, and the
    levels are `explain`'s. With the 22-cluster ligand of test_gpu_attribution.py::test_level_cap: 20 levels in every answer."""
    from pharmaconet_amd import PackedLibrary
    from pharmaconet_amd.engine import align, attribute, explain
    from pharmaconet_amd.library import LigandFeatures, pack_ligand

    model, lib, weights, ex, _ = posed("set_6oim_c8")
    i0 = next(i for i in range(len(ex)) if ex.status[i] == 0 and 2 <= len(ex.levels[i]) < 20)  # (below 20: a key has room for a match at level nl)
    pos = (np.asarray(model.flat.cluster_center).mean(axis=0) + np.random.default_rng(11).uniform(-5, 5, (22, 3, 3))).astype(np.float32)
    capped = None
    for ftype in ("Halogen", "Cation", "Anion", "HBond_acceptor", "HBond_donor"):
        one = PackedLibrary.from_records([pack_ligand(LigandFeatures([9] * 22, [[] for _ in range(22)], [(ftype, a, a) for a in range(22)], pos))])
        if one.header(0)[2] == 22 and candidates(model, one.unpack(0), 0):
            capped = one.record(0)
            break
    assert capped is not None
    both = PackedLibrary.from_records([lib.record(int(ex.indices[i0])), capped])
    ex2 = explain(model, both, [0, 1], weights=weights)
    assert ex2.status.tolist() == [0, 0] and ex2.levels[0].tolist() == ex.levels[i0].tolist() and len(ex2.levels[1]) == 20
    rec0 = both.unpack(0)
    nl, C = len(ex2.levels[0]), len(ex2.conf_max[0])
    c0, c1 = int(ex2.best_conformer[0]), int(ex2.best_conformer[1])
    key = ex2.match[0][c0]
    assert 2 <= nl < 20 and (key >= 0).any()
    l0 = int(np.flatnonzero(key >= 0)[0])
    stranger = key.copy()
    stranger[l0] = next(m for m in range(model.flat.num_clusters) if m not in candidates(model, rec0, int(ex2.levels[0][l0])))
    beyond = np.append(key, key[l0])  # a match at level nl
    none = np.full(nl, NONE, dtype=np.int64)
    rows = [(0, c0, key), (0, c0, none), (0, C, key), (0, -1, key), (0, c0, stranger), (0, c0, beyond), (len(both), 0, none), (1, c1, ex2.match[1][c1])]
    args = ([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
    at = attribute(model, both, *args, weights=weights)
    al = align(model, both, *args, weights=weights)
    assert at.status.tolist() == al.status.tolist() == [0, 0, 4, 4, 4, 4, 1, 0]
    for r, (lig, _, _) in enumerate(rows):
        assert at.levels[r].tolist() == al.levels[r].tolist() and len(at.node[r]) == len(al.node[r]), r
        if at.status[r] != 1:
            assert at.levels[r].tolist() == ex2.levels[lig].tolist() and len(at.node[r]) == both.header(lig)[0], r
    assert len(at.levels[6]) == len(at.node[6]) == 0 and len(at.levels[7]) == len(al.levels[7]) == 20


def test_limits_and_keys_that_are_no_leaf():
    from pharmaconet_amd.constants import weights_vector
    from pharmaconet_amd.engine import align
    from test_gpu_attribution import prefilter_margin

    model, lib, weights, ex, base = posed("set_6oim_c8")
    w7 = weights_vector(weights)
    empty = align(model, lib, [], [], [], weights=weights)
    assert len(empty) == 0 and empty.rotation.shape == (0, 3, 3) and empty.rmsd.size == 0
    with pytest.raises(ValueError):
        align(model, lib, np.zeros(65537, np.int64), np.zeros(65537, np.int64), [[]] * 65537, weights=weights)
    # two matches that the cluster-distance prefilter rejects for every conformer: candidates of their levels, no leaf of the tree
    found = None
    for i in range(len(ex)):
        if ex.status[i] != 0 or found:
            continue
        rec = lib.unpack(int(ex.indices[i]))
        T = Tables(model, rec, w7)
        lv = ex.levels[i]
        for l1 in range(len(lv)):
            for l2 in range(l1 + 1, len(lv)):
                for a1 in candidates(model, rec, int(lv[l1])):
                    for a2 in candidates(model, rec, int(lv[l2])):
                        if found is None and prefilter_margin(T, model, int(lv[l1]), a1, int(lv[l2]), a2) > 1.0:
                            found = (i, l1, a1, l2, a2)
    assert found is not None
    i, l1, a1, l2, a2 = found
    far = np.full(len(ex.levels[i]), NONE, dtype=np.int64)
    far[l1], far[l2] = a1, a2
    al = align(model, lib, [int(ex.indices[i])], [0], [far], weights=weights)
    rec = lib.unpack(int(ex.indices[i]))
    ref = align_ref.align(model, rec, w7, ex.levels[i], far, 0)
    assert al.status[0] == 0 and ref["n_pairs"] > 0
    check_row(al, 0, ref, 100.0, "no leaf")


def test_same_bits_twice():
    from pharmaconet_amd.engine import align

    model, lib, weights, ex, base = posed("set_6oim_c8")
    rows = np.asarray(base.rows)
    keys = [ex.match[i][c] for i, c in zip(rows, base.conformers)]
    # (with rows that are not OK: NaNs are compared as equal)
    idx = np.concatenate([base.indices, [len(lib), base.indices[0]]])
    conf = np.concatenate([base.conformers, [0, 64]])
    keys = keys + [[], keys[0]]
    first = align(model, lib, idx, conf, keys, weights=weights)
    second = align(model, lib, idx, conf, keys, weights=weights)
    assert first.status.tolist()[-2:] == [1, 4] and same_bits(first, second)
    assert all(np.array_equal(first.rotation[r], base.rotation[r]) and np.array_equal(first.node[r], base.node[r]) for r in range(len(base)))


# ---------------------------------------------------------------------------------------------------------------- the Python layer
def test_poses_of_explanations_and_modes():
    from pharmaconet_amd.engine import align, explain_modes

    model, lib, weights, ex, base = posed("set_c21_c8")
    rows = np.asarray(base.rows)
    direct = align(model, lib, ex.indices[rows], ex.best_conformer[rows], [ex.match[i][int(ex.best_conformer[i])] for i in rows], weights=weights)
    assert same_bits(direct, base) and np.array_equal(base.rows, rows)
    ms = explain_modes(model, lib, ex.indices, modes=2, weights=weights)
    p0, p1 = ms.explanation(0).poses(model, lib, weights=weights), ms.explanation(1).poses(model, lib, weights=weights)
    assert same_bits(p0, base) and len(p1) == len(p0)
    e0, e1 = ms.explanation(0), ms.explanation(1)
    differ = 0
    for r, i in enumerate(p1.rows):
        c = int(e1.best_conformer[i])
        k0, k1 = e0.match[i][c], e1.match[i][c]
        if p1.status[r] == 0 and p0.conformers[r] == c and (k1 >= 0).sum() >= 3 and not np.array_equal(k0, k1) and p1.gap[r] >= GATE * p1.scale[r] and p0.gap[r] >= GATE * p0.scale[r]:
            differ += 1
            assert not np.array_equal(p0.rotation[r], p1.rotation[r]) or not np.array_equal(p0.translation[r], p1.translation[r]), (i, k0, k1)
    assert differ > 0


def test_scoring_pose_and_type_weights():
    from pharmaconet_amd.constants import TYPE_NAMES, weights_vector
    from pharmaconet_amd.engine import align
    from test_attribution_cpu import load_mols

    model, lib, weights, ex, base = posed("set_6oim_c8")
    mols = load_mols("set_6oim_c8")
    r = next(r for r in range(len(base)) if base.n_nodes[r] >= 3)
    i = int(base.indices[r])
    pose = model.scoring_pose(mols[i], weights=weights)
    assert pose["status"] == 0 and pose["conformer"] == base.conformers[r] and np.array_equal(pose["rotation"], base.rotation[r])
    atoms = np.asarray(mols[i].atom_positions, dtype=np.float64)[:, int(base.conformers[r])]
    assert pose["positions"].shape == (mols[i].num_atoms, 3) and np.array_equal(pose["positions"], base.transform(r, atoms))
    assert np.array_equal(pose["positions"], atoms @ base.rotation[r].T + base.translation[r])
    packed = model.scoring_pose(lib.record(i), weights=weights, conformer=0, key=np.full(len(base.levels[r]), -1))
    assert packed["status"] == 0 and packed["positions"] is None and packed["n_pairs"] == 0 and np.array_equal(packed["rotation"], np.eye(3))
    # a zero type weight removes that type's pairs
    w = dict(zip(TYPE_NAMES, weights_vector(weights)))
    rec = lib.unpack(i)
    c, key = int(base.conformers[r]), ex.match[int(base.rows[r])][int(base.conformers[r])]
    dropped = 0
    for t in TYPE_NAMES:
        wz = dict(w, **{t: 0.0})
        ref = align_ref.align(model, rec, weights_vector(wz), base.levels[r], key, c)
        got = align(model, lib, [i], [c], [key], weights=wz)
        assert got.status[0] == 0 and (int(got.n_nodes[0]), int(got.n_pairs[0])) == (ref["n_nodes"], ref["n_pairs"])
        dropped += ref["n_pairs"] < base.n_pairs[r]
        check_row(got, 0, ref, 100.0, ("zero weight", t))
    assert dropped > 0


def test_cli_poses_csv(tmp_path):
    from pharmaconet_amd.engine import explain
    from pharmaconet_amd.screening import main

    model, lib, _, _ = load_golden("set_6oim_c8")
    libfile = tmp_path / "lib.pmxlib"
    lib.save(libfile)
    args = ["-p", str(GOLDEN / "model_6oim_like.pm"), "-d", str(libfile), "--explain", "5"]
    main(args + ["-o", str(tmp_path / "plain.csv"), "--explain_out", str(tmp_path / "plain_hits.csv")])
    main(args + ["-o", str(tmp_path / "with.csv"), "--explain_out", str(tmp_path / "hits.csv"), "--poses", str(tmp_path / "poses.csv")])
    assert (tmp_path / "plain.csv").read_bytes() == (tmp_path / "with.csv").read_bytes()
    assert (tmp_path / "plain_hits.csv").read_bytes() == (tmp_path / "hits.csv").read_bytes()
    with pytest.raises(SystemExit):
        main(["-p", str(GOLDEN / "model_6oim_like.pm"), "-d", str(libfile), "-o", str(tmp_path / "x.csv"), "--poses", str(tmp_path / "p.csv")])
    hits = [row.split(",") for row in (tmp_path / "hits.csv").read_text().splitlines()[1:]]
    rows = (tmp_path / "poses.csv").read_text().splitlines()
    assert rows[0] == "rank,path,conformer,rmsd,rmsd_nodes,fitted_nodes,r00,r01,r02,r10,r11,r12,r20,r21,r22,tx,ty,tz" and len(rows) == 6 == len(hits) + 1
    names = {f"{libfile}#{i}": i for i in range(len(lib))}
    idx = [names[h[1]] for h in hits]
    al = explain(model, lib, idx).poses(model, lib)  # (the command line's default weights are the engine's)
    for r, row in enumerate(rows[1:]):
        f = row.split(",")
        assert len(f) == 18 and int(f[0]) == r + 1 and f[1] == hits[r][1] and int(f[2]) == int(hits[r][3]) == al.conformers[r] and int(f[5]) == al.n_nodes[r]
        assert float(f[3]) == al.rmsd[r] and float(f[4]) == al.rmsd_nodes[r]
        assert np.array_equal(np.array([float(v) for v in f[6:15]]).reshape(3, 3), al.rotation[r]) and np.array_equal(np.array([float(v) for v in f[15:]]), al.translation[r])
        assert all(repr(float(v)) == v for v in f[3:5] + f[6:])
