"""`pmx_combo_overlay` on the GPU (csrc/pmx_colour.hip) against the NumPy restatement of tests/combo_ref.py over the seeded rows of
tests/combo_cases.py - every row a record of a library, its shape points a point set of its own or its nodes - the identities with
`pmx_shape_overlay`, `pmx_pose_colour` and `pmx_pose_shape` that must hold bit for bit, a golden hit with its atoms, repeatability,
statuses, the host's refusals, and the Python layer on top of it.

Bars. Integers (status, iterations, accepted steps, stop reason, shape points, nodes, features) must be equal; they can only differ where a
row stands within rounding of a decision, so they are asserted after the restatement's `decision_margin` is at least 1e-9 on every row
(the seeds are chosen so, checked on the CPU by tests/test_colour_cpu.py). Floats: the posed points - shape points and nodes - under the
returned motion and the relative final F are within max(1e-12, 1000 S), S = combo_cases.S[case] being how far rounding alone moves the
restatement over the very rows of the case: the project's bar for the Levenberg-Marquardt calls, for the sources the restatement does not
model - the device's exp, sin and cos."""

import ctypes
from functools import lru_cache

import numpy as np
import pytest

import combo_cases
import shape_ref
from combo_cases import COLOUR_RADIUS, COVER, FTOL, MARGIN, NODE_RADIUS
from conftest import load_golden
from test_gpu_pose_colour import case_ref as colour_case_ref

pytestmark = pytest.mark.gpu

EYE, ZERO = np.eye(3), np.zeros(3)
FIELDS = ("rotation", "translation", "overlap_start", "overlap", "self_overlap", "reference_overlap", "tanimoto_start", "tanimoto", "angle", "shift", "iterations", "accepted",
          "stop", "n_points", "start", "status", "colour_overlap_start", "colour_overlap", "colour_self_overlap", "colour_reference_overlap", "colour_tanimoto_start",
          "colour_tanimoto", "combo_start", "combo", "n_nodes", "n_reference_features")
FLOATS = ("overlap_start", "overlap", "self_overlap", "reference_overlap", "tanimoto_start", "tanimoto", "colour_overlap_start", "colour_overlap", "colour_self_overlap",
          "colour_reference_overlap", "colour_tanimoto_start", "colour_tanimoto", "combo_start", "combo", "angle", "shift")  # in the order of energy [16]


@lru_cache(maxsize=None)
def case_ref(name):
    from pharmaconet_amd.shape import ReferenceLigand

    c = combo_cases.case(name)
    ref = ReferenceLigand.from_arrays(c["ref_xyz"], c["ref_radius"])
    ref.colour = colour_case_ref(name)
    return ref


def source(c, rows):
    if c["points"] is None:
        return dict(node_radius=NODE_RADIUS)
    return dict(points=[c["points"][i] for i in rows], point_radii=[c["radii"][i] for i in rows], node_radius=NODE_RADIUS)


def run(name, rows=None, **kw):
    from pharmaconet_amd.engine import combo_overlay

    c = combo_cases.case(name)
    rows = list(range(c["n"])) if rows is None else [int(i) for i in rows]
    lib, conf = combo_cases.library(name)
    args = dict(colour_weight=c["cw"], ftol=FTOL, max_iter=c["max_iter"], rotation=c["R"][rows], translation=c["t"][rows])
    args.update(source(c, rows))
    args.update(kw)
    return combo_overlay(case_ref(name), lib, rows, conf[rows], **args)


@lru_cache(maxsize=None)
def result(name):
    return run(name)


def same_bits(a, b, rows=None):
    rows = np.arange(len(b)) if rows is None else np.asarray(rows)
    return len(a) == len(rows) and all(np.array_equal(getattr(a, f), getattr(b, f)[rows], equal_nan=True) for f in FIELDS)


def objective(out, cw):
    """F at the start and at the end from the device's own overlaps: the kernel's expression, so the same bits."""
    return out.overlap_start + np.float64(cw) * out.colour_overlap_start, out.overlap + np.float64(cw) * out.colour_overlap


def check_against(out, ref, c, rows, tag, bar):
    """Every row of `out` against the restatement's rows; the figures are printed before they are asserted."""
    assert len(out) == len(ref), tag
    margin = min([r["decision_margin"] for r in ref], default=np.inf)
    f_end = objective(out, c["cw"])[1]
    worst_p = worst_f = 0.0
    for k, r in enumerate(ref):
        if r["status"] != 0 or out.status[k] != 0:
            continue
        both = np.concatenate([np.asarray(combo_cases.shape_points(c, rows[k])[0], np.float32).reshape(-1, 3), c["nodes"][rows[k]].reshape(-1, 3)])
        if len(both):
            worst_p = max(worst_p, float(np.abs(shape_ref.pose(both, out.rotation[k], out.translation[k]) - shape_ref.pose(both, r["rotation"], r["translation"])).max()))
        if r["F"][1] > 0:
            worst_f = max(worst_f, abs(f_end[k] - r["F"][1]) / r["F"][1])
    print(f"{tag}: rows {len(ref)} decision margin {margin:.3e} worst posed point error {worst_p:.3e} A, worst relative F error {worst_f:.3e} (bar {bar:.1e})")
    assert margin >= MARGIN, (tag, margin)
    for k, r in enumerate(ref):
        got = [int(out.status[k]), int(out.iterations[k]), int(out.accepted[k]), int(out.stop[k]), int(out.n_points[k]), int(out.n_nodes[k]), int(out.n_reference_features[k])]
        assert got == [int(r["status"])] + [int(v) for v in r["count"]], (tag, k, got, r["count"])
    assert worst_p <= bar and worst_f <= bar, (tag, worst_p, worst_f, bar)
    # the other floats, loosely: they are functions of the motion and the overlaps checked above
    for k, r in enumerate(ref):
        if r["status"] == 0:
            got = np.array([getattr(out, f)[k] for f in FLOATS])
            assert np.allclose(got, r["energy"], rtol=1e-6, atol=1e-7), (tag, k, got, r["energy"])


def check_identities(out, name, rows, tag, start_R, start_t):
    """What must hold bit for bit against `pmx_pose_colour` and `pmx_pose_shape`, and the properties of every row."""
    from pharmaconet_amd.engine import colour, shape

    c = combo_cases.case(name)
    lib, conf = combo_cases.library(name)
    ref = case_ref(name)
    ok = out.status == 0
    end_R, end_t = np.where(ok[:, None, None], out.rotation, 0.0), np.where(ok[:, None], out.translation, 0.0)
    if c["points"] is None:
        shape_source = dict(library=lib, indices=rows, conformers=conf[rows], node_radius=NODE_RADIUS)
    else:
        shape_source = dict(points=[c["points"][i] for i in rows], point_radii=[c["radii"][i] for i in rows])
    s0, s1 = shape(ref, rotation=start_R, translation=start_t, **shape_source), shape(ref, rotation=end_R, translation=end_t, **shape_source)
    c0, c1 = colour(ref, lib, rows, conf[rows], start_R, start_t, cover=COVER), colour(ref, lib, rows, conf[rows], end_R, end_t, cover=COVER)
    assert np.array_equal(s0.status == 0, ok) and np.array_equal(c0.status == 0, ok), tag
    assert np.array_equal(out.overlap_start[ok], s0.overlap[ok]) and np.array_equal(out.overlap[ok], s1.overlap[ok]) and np.array_equal(out.self_overlap[ok], s0.self_overlap[ok]), tag
    assert np.array_equal(out.reference_overlap[ok], s0.reference_overlap[ok]) and np.array_equal(out.tanimoto_start[ok], s0.tanimoto[ok]), tag
    assert np.array_equal(out.colour_overlap_start[ok], c0.overlap[ok]) and np.array_equal(out.colour_overlap[ok], c1.overlap[ok]), tag
    assert np.array_equal(out.colour_self_overlap[ok], c0.self_overlap[ok]) and np.array_equal(out.colour_reference_overlap[ok], c0.reference_overlap[ok]), tag
    assert np.array_equal(out.colour_tanimoto_start[ok], c0.tanimoto[ok]) and np.array_equal(out.n_points[ok], s0.n_points[ok]) and np.array_equal(out.n_nodes[ok], c0.n_nodes[ok]), tag
    assert np.array_equal(out.combo_start[ok], out.tanimoto_start[ok] + out.colour_tanimoto_start[ok]) and np.array_equal(out.combo[ok], out.tanimoto[ok] + out.colour_tanimoto[ok]), tag
    assert ((out.combo[ok] >= 0) & (out.combo[ok] <= 2 + 1e-12)).all(), tag
    f0, f1 = objective(out, out.colour_weight)
    moved = ok & (out.accepted > 0)
    assert (f1[ok] >= f0[ok]).all() and (f1[moved] > f0[moved]).all(), tag
    nothing = ok & (f0 == 0)
    assert (out.stop[nothing] == 0).all() and (out.iterations[nothing] == 0).all() and (out.stop[ok & ~nothing] > 0).all(), tag
    same = ok & (out.accepted == 0)
    assert np.array_equal(out.rotation[same], np.asarray(start_R)[same]) and np.array_equal(out.translation[same], np.asarray(start_t)[same]), tag
    assert (out.angle[same] == 0).all() and (out.shift[same] == 0).all(), tag
    bad = ~ok
    assert np.isnan(out.rotation[bad]).all() and np.isnan(out.translation[bad]).all() and (out.stop[bad] == -1).all(), tag
    for f in ("iterations", "accepted", "n_points", "n_nodes", "n_reference_features"):
        assert (getattr(out, f)[bad] == 0).all(), (tag, f)
    for f in FLOATS:
        assert np.isnan(getattr(out, f)[bad]).all() and np.isfinite(getattr(out, f)[ok]).all(), (tag, f)
    R = out.rotation[ok]
    assert np.abs(np.einsum("nji,njk->nik", R, R) - np.eye(3)).max(initial=0.0) <= 1e-12 and (np.linalg.det(R) > 0).all(), tag


# ---------------------------------------------------------------------------------------------------------------- 1. against the restatement
@pytest.mark.parametrize("name", list(combo_cases.CASES))
def test_every_case_against_the_restatement(name):
    c = combo_cases.case(name)
    out = result(name)
    rows = list(range(c["n"]))
    check_against(out, combo_cases.reference(name), c, rows, name, combo_cases.bar(name))
    check_identities(out, name, rows, name, c["R"], c["t"])
    assert (out.start == -1).all() and out.start_tanimoto.shape == (c["n"], 0) and np.array_equal(out.indices, rows) and out.colour_weight == c["cw"]
    if c["max_iter"] == 0:
        assert np.array_equal(out.rotation, c["R"]) and np.array_equal(out.translation, c["t"]) and set(out.stop.tolist()) <= {0, 2}
    elif c["max_iter"] > 1:
        assert (out.accepted > 0).sum() >= 50


def test_colour_weight_zero_is_the_shape_overlay():
    """Motions, O_AB, iterations, accepted steps and the stop reason are `pmx_shape_overlay`'s on the same rows, bit for bit - with a point
    set per row, and with the nodes as the shape points."""
    from pharmaconet_amd.engine import overlay

    for name in ("cw0", "f2_nodes"):
        c = combo_cases.case(name)
        rows = list(range(c["n"]))
        lib, conf = combo_cases.library(name)
        out = result(name) if c["cw"] == 0 else run(name, colour_weight=0.0)
        if c["points"] is None:
            sh = overlay(case_ref(name), lib, rows, conf, c["R"], c["t"], node_radius=NODE_RADIUS, ftol=FTOL, max_iter=c["max_iter"])
        else:
            sh = overlay(case_ref(name), rotation=c["R"], translation=c["t"], points=c["points"], point_radii=c["radii"], ftol=FTOL, max_iter=c["max_iter"])
        for f in FIELDS[:16]:
            if f != "start":
                assert np.array_equal(getattr(out, f), getattr(sh, f), equal_nan=True), (name, f)
        assert (out.accepted > 0).sum() >= 40 and (out.colour_overlap != out.colour_overlap_start).any(), name


def test_a_golden_hit_on_itself_has_combo_two_and_finds_its_way_back():
    """`ReferenceLigand.from_library` of a golden hit with its atoms: overlaid from the identity it has combo exactly 2.0 at the start; moved
    a little it comes back. With "balanced" the weight is O_BB / C_BB of the two handles."""
    from pharmaconet_amd.atoms import PackedAtoms
    from pharmaconet_amd.engine import balanced_colour_weight, combo_overlay, device_colour_ref, device_shape_ref
    from pharmaconet_amd.shape import ReferenceLigand
    from test_attribution_cpu import load_mols

    _, lib, _, _ = load_golden("set_6oim_c8")
    store = PackedAtoms.for_library(load_mols("set_6oim_c8"), lib)
    hit, conf = 5, 1
    ref = ReferenceLigand.from_library(lib, hit, conf, atoms=store)
    shift = shape_ref.random_rotations(np.random.default_rng(4), 1)[0]
    axis = np.array([0.3, -0.2, 0.1])
    from overlay_cases import rotation_about

    centre = ref.xyz.astype(np.float64).mean(axis=0)
    Rm = rotation_about(axis, 0.25)
    out = combo_overlay(ref, lib, [hit, hit, hit + 1], [conf, conf, 0], [EYE, Rm, shift], [ZERO, centre - Rm @ centre + 0.5, ZERO], atoms=store, max_iter=64, ftol=1e-9)
    assert out.status.tolist() == [0, 0, 0] and out.combo_start[0] == 2.0 and out.tanimoto_start[0] == 1.0 and out.colour_tanimoto_start[0] == 1.0
    assert out.overlap_start[0] == out.self_overlap[0] == out.reference_overlap[0] and out.colour_overlap_start[0] == out.colour_self_overlap[0] == out.colour_reference_overlap[0]
    assert out.n_points[0] == len(ref) and out.n_nodes[0] == len(ref.colour) == out.n_reference_features[0]
    w = device_shape_ref(ref).self_overlap / device_colour_ref(ref).self_overlap
    assert out.colour_weight == w == balanced_colour_weight(ref) and w > 0
    print(f"a moved copy: combo {out.combo_start[1]:.4f} -> {out.combo[1]:.9f} in {out.iterations[1]} trials; another ligand: {out.combo_start[2]:.4f} -> {out.combo[2]:.4f}")
    assert out.combo_start[1] < 1.6 and out.combo[1] > 2.0 - 1e-6 and out.combo[2] >= out.combo_start[2] - 1e-12 and out.combo[2] < 2.0
    # the nodes as the shape points, and the posed rows' own method
    nodes = ReferenceLigand.from_library(lib, hit, conf, node_radius=NODE_RADIUS)
    own = combo_overlay(nodes, lib, [hit], [conf], [EYE], [ZERO], node_radius=NODE_RADIUS)
    assert own.combo_start[0] == 2.0 and own.n_points[0] == own.n_nodes[0]
    # posed rows overlay themselves: `combo_overlay_of` the motions found above starts where they ended
    from pharmaconet_amd.engine import Alignment, combo_overlay_of

    al = Alignment(indices=out.indices, conformers=out.conformers, rotation=out.rotation, translation=out.translation, rmsd=None, rmsd_nodes=None, weight=None, sse=None, scale=None,
                   gap=None, node=None, n_nodes=None, n_pairs=None, levels=None, status=out.status)
    again = combo_overlay_of(al, ref, lib, atoms=store, max_iter=64, ftol=1e-9)
    assert np.array_equal(again.overlap_start, out.overlap) and np.array_equal(again.colour_overlap_start, out.colour_overlap) and np.array_equal(again.indices, out.indices)
    with pytest.raises(ValueError):
        combo_overlay_of(al, ref, lib, starts=4)


def test_four_starts_keep_the_highest_combo_and_the_lower_among_equals():
    from pharmaconet_amd.engine import combo_overlay, overlay_starts

    name = "f63"
    c = combo_cases.case(name)
    lib, conf = combo_cases.library(name)
    rows = [10, 0, 12, 21]  # (row 0 has no node)
    pts, rad = [c["points"][i] for i in rows], [c["radii"][i] for i in rows]
    out = combo_overlay(case_ref(name), lib, rows, conf[rows], starts=4, points=pts, point_radii=rad, colour_weight=c["cw"], ftol=FTOL)
    assert len(out) == 4 and out.start_tanimoto.shape == (4, 4) and (out.status == 0).all()
    assert np.array_equal(out.start, np.argmax(out.start_tanimoto, axis=1)) and np.array_equal(out.combo, out.start_tanimoto[np.arange(4), out.start])
    st = overlay_starts(case_ref(name), out.start, points=pts)
    again = combo_overlay(case_ref(name), lib, rows, conf[rows], st.rotation, st.translation, points=pts, point_radii=rad, colour_weight=c["cw"], ftol=FTOL)
    for f in FIELDS:
        if f != "start":
            assert np.array_equal(getattr(again, f), getattr(out, f)), f
    with pytest.raises(ValueError):
        combo_overlay(case_ref(name), lib, rows, conf[rows], starts=2)
    with pytest.raises(ValueError):
        combo_overlay(case_ref(name), lib, [0] * 16385, [1] * 16385, starts=4)


# ---------------------------------------------------------------------------------------------------------------- 2. repeatability
@pytest.mark.parametrize("n", [1, 4, 5, 64])
def test_row_counts_and_the_same_bits_wherever_a_row_stands(n):
    name = "f63"
    c = combo_cases.case(name)
    whole = result(name)
    big = int(np.flatnonzero([len(p) == 256 for p in c["points"]])[0])
    pick = [i % 64 for i in ([big, 2, 12, 5, 0] + list(range(13, 72)))[:n]]  # (256 points first: the longest row of the call stands in wave 0)
    out = run(name, rows=pick)
    assert same_bits(out, whole, rows=pick)
    assert same_bits(run(name, rows=pick), out)  # two runs
    if n == 64:
        moving = int(np.flatnonzero(whole.accepted > 2)[0])
        rows = [moving] + list(range(5)) + [moving] * 3 + list(range(5, 9)) + [moving]  # first, repeated, last
        assert same_bits(run(name, rows=rows), whole, rows=rows)


# ---------------------------------------------------------------------------------------------------------------- 3. rows that are not OK
def test_every_status_that_is_not_ok():
    from pharmaconet_amd.engine import combo_overlay

    name = "f63"
    c = combo_cases.case(name)
    ref = case_ref(name)
    lib, conf = combo_cases.library(name)
    bad_R = EYE.copy()
    bad_R[2, 0] = np.inf
    p3, r3 = c["points"][3], c["radii"][3]
    neg = r3.copy()
    neg[1] = -1.0
    idx, cf = [3, 3, 3, 64, 3, 3, 3], [1, 2, -1, 1, 1, 1, 1]
    R = [EYE, EYE, EYE, EYE, bad_R, EYE, EYE]
    pts, rad = [p3] * 5 + [np.zeros((257, 3), np.float32), p3], [r3] * 5 + [np.ones(257, np.float32), neg]
    out = combo_overlay(ref, lib, idx, cf, R, [ZERO] * 7, points=pts, point_radii=rad, colour_weight=1.0)
    assert out.status.tolist() == [0, 4, 4, 1, 4, 1, 4]
    bad = out.status != 0
    assert np.isnan(out.rotation[bad]).all() and np.isnan(out.translation[bad]).all() and (out.stop[bad] == -1).all()
    for f in FLOATS:
        assert np.isnan(getattr(out, f)[1:]).all() and np.isfinite(getattr(out, f)[0]), f
    for f in ("iterations", "accepted", "n_points", "n_nodes", "n_reference_features"):
        assert (getattr(out, f)[1:] == 0).all(), f
    assert same_bits(combo_overlay(ref, lib, [3], [1], [EYE], [ZERO], points=[p3], point_radii=[r3], colour_weight=1.0), out, rows=[0])
    # the nodes as the shape points: a radius that is none
    nodes = combo_overlay(ref, lib, [3, 3], [1, 1], [EYE, EYE], [ZERO, ZERO], node_radius=0.0, colour_weight=1.0)
    assert nodes.status.tolist() == [4, 4]
    # a record with a mask of 128: the upload neutralises it (pmx_library_upload), so the row is unsupported before the kernel's own rule is reached
    from pharmaconet_amd import PackedLibrary

    masks = c["masks"][3].copy()
    masks[5] = 128
    odd = PackedLibrary.from_records([combo_cases.record(c["nodes"][3], masks), combo_cases.record(c["nodes"][3], c["masks"][3])])
    got = combo_overlay(ref, odd, [0, 1], [1, 1], [EYE, EYE], [ZERO, ZERO], points=[p3, p3], point_radii=[r3, r3], colour_weight=1.0)
    assert got.status.tolist() == [1, 0] and np.isnan(got.combo[0]) and got.overlap[1] == out.overlap[0] and np.array_equal(got.rotation[1], out.rotation[0])


def test_rows_the_atom_store_has_nothing_for():
    from pharmaconet_amd.atoms import PackedAtoms
    from pharmaconet_amd.engine import combo_overlay

    name = "f63"
    c = combo_cases.case(name)
    lib, conf = combo_cases.library(name)
    rng = np.random.default_rng(6)
    zs = [np.full(9, 6), np.zeros(0, np.int64), np.full(5, 8)]
    ps = [rng.normal(size=(9, 2, 3)).astype(np.float32) + 2.0, np.zeros((0, 2, 3), np.float32), rng.normal(size=(5, 1, 3)).astype(np.float32)]
    store = PackedAtoms.from_arrays(zs, ps)
    three = lib.select([3, 5, 7])
    out = combo_overlay(case_ref(name), three, [0, 1, 2, 0], [1, 1, 1, 1], [EYE] * 4, [c["t"][3]] * 4, atoms=store, colour_weight=1.0)
    assert out.status[0] == 0 and out.status[3] == 0 and out.status[1] != 0 and out.status[2] == 4 and out.n_points[0] == 9  # (no atoms; no such conformer in the store)
    assert np.isnan(out.rotation[1]).all() and np.isnan(out.combo[2])
    by_points = combo_overlay(case_ref(name), three, [0], [1], [EYE], [c["t"][3]], points=[ps[0][:, 1]], point_radii=[np.full(9, 1.7, np.float32)], colour_weight=1.0)
    assert np.array_equal(by_points.rotation[0], out.rotation[0]) and by_points.combo[0] == out.combo[0] == out.combo[3]


@pytest.mark.parametrize("n", [1, 4, 5])  # a lone row, a full block, a block and a tail
def test_the_atom_store_is_the_same_atoms_as_points(n):
    """Rows whose shape points the store gathers on the device, and the same rows with the same atoms and Bondi radii as `points` /
    `point_radii`: the same bits in every field, from the given motions and from the four starts. A row the store has no atoms for is
    not OK in the store's call (as points it is an OK row without a point, so it is left out of the comparison)."""
    from pharmaconet_amd.atoms import PackedAtoms
    from pharmaconet_amd.engine import combo_overlay
    from pharmaconet_amd.pocket import atomic_number_radii

    name = "f63"
    c = combo_cases.case(name)
    lib, _ = combo_cases.library(name)
    rng = np.random.default_rng(6)
    zs = [np.full(9, 6), np.zeros(0, np.int64), np.array([8, 6, 7, 6, 16])]
    ps = [rng.normal(size=(9, 2, 3)).astype(np.float32) + 2.0, np.zeros((0, 2, 3), np.float32), rng.normal(size=(5, 2, 3)).astype(np.float32) + 2.0]
    store = PackedAtoms.from_arrays(zs, ps)
    three = lib.select([3, 5, 7])
    idx, cf = np.array([0, 1, 2, 0, 2][:n]), np.array([1, 1, 0, 0, 1][:n])  # (ligand 1: no atoms)
    pts = [ps[i][:, k] for i, k in zip(idx, cf)]
    rad = [np.asarray(atomic_number_radii(zs[i]), np.float32) for i in idx]
    bad = idx == 1
    for starts, motion in ((0, dict(rotation=[EYE] * n, translation=[c["t"][3]] * n)), (4, {})):
        by_store = combo_overlay(case_ref(name), three, idx, cf, atoms=store, starts=starts, colour_weight=1.0, **motion)
        by_points = combo_overlay(case_ref(name), three, idx, cf, points=pts, point_radii=rad, starts=starts, colour_weight=1.0, **motion)
        assert len(by_store) == len(by_points) == n and (by_store.status[~bad] == 0).all() and (by_store.n_points[~bad] == [len(p) for p, b in zip(pts, bad) if not b]).all(), starts
        for f in FIELDS:
            assert np.array_equal(getattr(by_store, f)[~bad], getattr(by_points, f)[~bad], equal_nan=True), (starts, f)
        assert (by_store.status[bad] == 1).all() and (by_store.stop[bad] == -1).all() and (by_store.n_points[bad] == 0).all(), starts
        assert np.isnan(by_store.rotation[bad]).all() and np.isnan(by_store.translation[bad]).all() and all(np.isnan(getattr(by_store, f)[bad]).all() for f in FLOATS), starts
        assert by_store.start_tanimoto.shape == (n, starts) and (np.isnan(by_store.start_tanimoto[bad]).all() if starts else True)


def test_the_hosts_refusals_and_no_rows():
    import torch

    from pharmaconet_amd import _ffi
    from pharmaconet_amd.engine import combo_overlay, device_colour_ref, device_shape_ref

    name = "f63"
    c = combo_cases.case(name)
    ref = case_ref(name)
    packed, conf = combo_cases.library(name)
    lib = _ffi.load()
    sh, co = device_shape_ref(ref, 0), device_colour_ref(ref, 0)
    dev = torch.device("cuda", 0)
    z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=dev)  # noqa: E731
    from pharmaconet_amd.engine import DeviceLibrary

    dlib = DeviceLibrary(packed, 0)
    try:
        lig, cf, rot, trans = z(1, dt=torch.int64), z(1, dt=torch.int32) + 1, z(1, 9), z(1, 3)
        outs = [z(1, 9), z(1, 3), z(1, 16), z(1, 6, dt=torch.int32), z(1, dt=torch.int32)]
        ptrs = [o.data_ptr() for o in outs]

        def call(shape=sh.handle, colour=co.handle, library=dlib.handle, n=1, cw=1.0, ftol=1e-6, max_iter=8, triple=(None, None, None), radius=1.0, o=ptrs):
            return lib.pmx_combo_overlay(shape, colour, library, lig.data_ptr(), cf.data_ptr(), *triple, rot.data_ptr(), trans.data_ptr(), n, radius, cw, ftol, max_iter, *o, None)

        assert call(shape=None) != 0 and b"null shape reference" in lib.pmx_last_error()
        assert call(colour=None) != 0 and b"null colour reference" in lib.pmx_last_error()
        assert call(library=None) != 0 and b"null library" in lib.pmx_last_error()
        assert call(n=65537) != 0 and call(cw=-1.0) != 0 and call(cw=float("nan")) != 0 and call(ftol=-1.0) != 0 and call(max_iter=65) != 0 and call(max_iter=-1) != 0
        assert call(radius=float("nan")) != 0 and call(o=[None] + ptrs[1:]) != 0 and call(o=ptrs[:-1] + [None]) != 0
        off = z(2, dt=torch.int64)
        assert call(triple=(off.data_ptr(), None, None)) != 0  # half a point triple
        assert call(n=0, o=[None] * 5) == 0  # n = 0 succeeds and writes nothing
        if torch.cuda.device_count() > 1:
            assert call(colour=device_colour_ref(ref, 1).handle) != 0 and b"on device" in lib.pmx_last_error()
        assert call() == 0  # (rot = 0: every point at the origin; finite, so the row is OK)
        torch.cuda.synchronize()
        assert int(outs[4].cpu()[0]) == 0 and outs[3].cpu()[0, 3:].tolist() == [0, 0, len(c["feat_mask"])]  # record 0 has no node
    finally:
        dlib.close()
    empty = combo_overlay(ref, packed, [], [], np.zeros((0, 3, 3)), np.zeros((0, 3)))
    assert len(empty) == 0 and empty.combo.shape == (0,) and empty.rotation.shape == (0, 3, 3)
    for kw in (dict(colour_weight=-1.0), dict(colour_weight="heavy"), dict(colour_weight=float("nan")), dict(max_iter=65), dict(ftol=-1.0), dict(node_radius=float("inf")),
               dict(point_radii=[c["radii"][3]]), dict(points=[c["points"][3]] * 2), dict(atoms=[1, 2])):
        with pytest.raises(ValueError):
            combo_overlay(ref, packed, [3], [1], [EYE], [ZERO], **kw)
    with pytest.raises(ValueError, match="library is required"):
        combo_overlay(ref, None, [3], [1], [EYE], [ZERO])
    with pytest.raises(ValueError):
        combo_overlay(ref, packed, [3], [1])  # starts=0 without motions
    from pharmaconet_amd.shape import ReferenceLigand

    with pytest.raises(ValueError, match="typed features"):
        combo_overlay(ReferenceLigand.from_arrays(c["ref_xyz"], c["ref_radius"]), packed, [3], [1], [EYE], [ZERO])
    bare = combo_overlay(ReferenceLigand.from_arrays(c["ref_xyz"], c["ref_radius"]), packed, [3], [1], [c["R"][3]], [c["t"][3]], colour=colour_case_ref(name), colour_weight=c["cw"],
                         ftol=FTOL, **source(c, [3]))
    assert same_bits(bare, result(name), rows=[3])
