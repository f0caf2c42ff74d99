"""`pmx_shape_overlay` and `pmx_shape_starts` on the GPU (csrc/pmx_shape_overlay.hip) against the NumPy restatement of tests/overlay_ref.py
over the seeded rows of tests/overlay_cases.py: point mode over the point counts and reference sizes at which the kernel's trips change, node
mode on a golden set, the atom store, the identities with `pmx_pose_shape` that must hold bit for bit, repeatability, statuses, the host's
refusals, and the Python layer and the command line on top of it.

Bars. Integers (status, iterations, accepted steps, stop reason, points) must be equal; they can only differ where a row stands within
rounding of a decision, so they are asserted after the restatement's `decision_margin` is at least 1e-9 on every row (the seeds are chosen
so, checked on the CPU by tests/test_overlay_cpu.py). Floats: the posed points under the returned motion and the relative final O_AB are
within max(1e-12, 1000 S), S = overlay_cases.S[case] being how far rounding alone moves the restatement over the very rows of the case; the
factor is the one the refinement's tests use, for the same unmodelled sources - the device's exp, sin and cos. The start motions use only
+ - * / and sqrt: bit equality is expected, a difference of at most 1e-12 is asserted, and the worst is printed."""

import ctypes
from functools import lru_cache

import numpy as np
import pytest

import overlay_cases
import overlay_ref
import shape_ref
from conftest import GOLDEN, load_golden
from overlay_cases import FTOL, MARGIN, NODE_RADIUS

pytestmark = pytest.mark.gpu

EYE, ZERO = np.eye(3), np.zeros(3)
FIELDS = ("rotation", "translation", "overlap_start", "overlap", "self_overlap", "reference_overlap", "tanimoto_start", "tanimoto", "angle", "shift", "iterations", "accepted",
          "stop", "n_points", "start", "status")


@lru_cache(maxsize=None)
def case_ref(name):
    from pharmaconet_amd.shape import ReferenceLigand

    c = overlay_cases.flat_case() if name == "flat" else overlay_cases.case(name)
    return ReferenceLigand.from_arrays(c["ref_xyz"], c["ref_radius"])


def golden_reference():
    return case_ref("flat")  # the 6OIM ligand


def run(name, rows=None, **kw):
    from pharmaconet_amd.engine import overlay

    c = overlay_cases.flat_case() if name == "flat" else overlay_cases.case(name)
    rows = list(range(c["n"])) if rows is None else list(rows)
    pick = lambda v: None if v is None else [v[i] for i in rows]  # noqa: E731
    args = dict(node_radius=NODE_RADIUS, ftol=FTOL, max_iter=c["max_iter"])
    args.update(kw)
    return overlay(case_ref(name), rotation=c["R"][rows], translation=c["t"][rows], points=pick(c["points"]), point_radii=pick(c["radii"]), **args)


@lru_cache(maxsize=None)
def result(name):
    return run(name)


def same_bits(a, b, rows=None):
    rows = np.arange(len(b)) if rows is None else np.asarray(rows)
    return len(a) == len(rows) and all(np.array_equal(getattr(a, f), getattr(b, f)[rows], equal_nan=True) for f in FIELDS)


def check_against(out, ref, points, tag, bar):
    """Every row of `out` against the restatement's rows; the figures are printed before they are asserted."""
    assert len(out) == len(ref), tag
    margin = min([r["decision_margin"] for r in ref], default=np.inf)
    worst_p = worst_o = 0.0
    for i, r in enumerate(ref):
        if r["status"] != 0 or out.status[i] != 0:
            continue
        if len(points[i]):
            worst_p = max(worst_p, float(np.abs(shape_ref.pose(points[i], out.rotation[i], out.translation[i]) - shape_ref.pose(points[i], r["rotation"], r["translation"])).max()))
        if r["energy"][1] > 0:
            worst_o = max(worst_o, abs(out.overlap[i] - r["energy"][1]) / r["energy"][1])
    print(f"{tag}: rows {len(ref)} decision margin {margin:.3e} worst posed point error {worst_p:.3e} A, worst relative O_AB error {worst_o:.3e} (bar {bar:.1e})")
    assert margin >= MARGIN, (tag, margin)
    for i, r in enumerate(ref):
        got = [int(out.status[i]), int(out.iterations[i]), int(out.accepted[i]), int(out.stop[i]), int(out.n_points[i])]
        assert got == [int(r["status"])] + [int(v) for v in r["count"]], (tag, i, got, r["count"])
    assert worst_p <= bar and worst_o <= bar, (tag, worst_p, worst_o, bar)
    # the other floats, loosely: they are functions of the motion and the overlaps checked above
    for i, r in enumerate(ref):
        if r["status"] == 0:
            got = np.array([out.overlap_start[i], out.overlap[i], out.self_overlap[i], out.reference_overlap[i], out.tanimoto_start[i], out.tanimoto[i], out.angle[i], out.shift[i]])
            assert np.allclose(got, r["energy"], rtol=1e-6, atol=1e-7), (tag, i, got, r["energy"])


def check_identities(out, reference, source, tag, start_R, start_t, **kw):
    """What must hold bit for bit against `pmx_pose_shape`, and the properties of every row."""
    from pharmaconet_amd.engine import shape

    ok = out.status == 0
    before = shape(reference, rotation=start_R, translation=start_t, **source, **kw)
    after = shape(reference, rotation=np.where(ok[:, None, None], out.rotation, 0.0), translation=np.where(ok[:, None], out.translation, 0.0), **source, **kw)
    assert np.array_equal(before.status == 0, ok), tag
    assert np.array_equal(out.overlap_start[ok], before.overlap[ok]) and np.array_equal(out.self_overlap[ok], before.self_overlap[ok]), tag
    assert np.array_equal(out.tanimoto_start[ok], before.tanimoto[ok]) and np.array_equal(out.reference_overlap[ok], before.reference_overlap[ok]), tag
    assert np.array_equal(out.overlap[ok], after.overlap[ok]) and np.array_equal(out.n_points[ok], before.n_points[ok]), tag
    assert (out.overlap[ok] >= out.overlap_start[ok]).all() and (out.overlap[ok & (out.accepted > 0)] > out.overlap_start[ok & (out.accepted > 0)]).all(), tag
    nothing = ok & ((out.n_points == 0) | (out.overlap_start == 0))
    assert (out.stop[nothing] == 0).all() and (out.iterations[nothing] == 0).all() and (out.stop[ok & ~nothing] > 0).all(), tag
    same = ok & (out.accepted == 0)
    assert np.array_equal(out.rotation[same], np.asarray(start_R)[same]) and np.array_equal(out.translation[same], np.asarray(start_t)[same]), tag
    assert (out.angle[same] == 0).all() and (out.shift[same] == 0).all(), tag
    bad = ~ok
    assert np.isnan(out.rotation[bad]).all() and np.isnan(out.translation[bad]).all() and (out.stop[bad] == -1).all(), tag
    assert (out.iterations[bad] == 0).all() and (out.accepted[bad] == 0).all() and (out.n_points[bad] == 0).all(), tag
    for f in FIELDS[2:10]:
        assert np.isnan(getattr(out, f)[bad]).all() and np.isfinite(getattr(out, f)[ok]).all(), (tag, f)
    R = out.rotation[ok]
    assert np.abs(np.einsum("nji,njk->nik", R, R) - np.eye(3)).max(initial=0.0) <= 1e-12 and (np.linalg.det(R) > 0).all(), tag
    return before, after


def variants_apart(refs, points):
    """S of rows that are no seeded case: how far the restatement's three variants (`refs[variant][row]`) lie apart in posed points and in
    relative final O_AB - after all three agree in every integer and stand 1e-9 off every decision."""
    s = 0.0
    for r, mine in enumerate(refs["forward"]):
        for v in ("reverse", "jitter"):
            other = refs[v][r]
            assert other["status"] == mine["status"] and np.array_equal(other["count"], mine["count"]) and other["decision_margin"] >= MARGIN, (r, v, other["decision_margin"])
            if mine["status"] == 0:
                s = max(s, float(np.abs(shape_ref.pose(points[r], other["rotation"], other["translation"]) - shape_ref.pose(points[r], mine["rotation"], mine["translation"])).max(initial=0.0)))
                s = max(s, abs(other["energy"][1] - mine["energy"][1]) / mine["energy"][1] if mine["energy"][1] > 0 else 0.0)
    return s


# ---------------------------------------------------------------------------------------------------------------- 1. point mode, every case
@pytest.mark.parametrize("name", list(overlay_cases.CASES))
def test_point_mode_against_the_restatement(name):
    c = overlay_cases.case(name)
    out = result(name)
    check_against(out, overlay_cases.reference(name), c["points"], name, overlay_cases.bar(name))
    check_identities(out, case_ref(name), dict(points=c["points"], point_radii=c["radii"], node_radius=NODE_RADIUS), name, c["R"], c["t"])
    assert (out.start == -1).all() and out.start_tanimoto.shape == (c["n"], 0) and out.indices is None
    if c["max_iter"] == 0:
        assert np.array_equal(out.rotation, c["R"]) and np.array_equal(out.translation, c["t"]) and set(out.stop.tolist()) == {0, 2}
    else:
        assert (out.accepted > 0).sum() >= 50


def test_rows_with_nothing_to_follow():
    c = overlay_cases.flat_case()
    out = run("flat")
    far, top = c["far"], c["at_maximum"]
    assert (out.status == 0).all()
    assert (out.stop[far] == 0).all() and (out.iterations[far] == 0).all() and (out.overlap[far] == 0).all() and (out.tanimoto[far] == 0).all()
    assert np.array_equal(out.rotation[far], c["R"][far]) and np.array_equal(out.translation[far], c["t"][far])
    # the reference's own atoms in place: Tanimoto exactly 1 at the start, and nothing to gain
    assert (out.overlap_start[top] == out.self_overlap[top]).all() and (out.self_overlap[top] == out.reference_overlap[top]).all() and (out.tanimoto_start[top] == 1.0).all()
    assert (out.overlap[top] >= out.overlap_start[top]).all() and (out.shift[top] <= 1e-6).all() and (out.stop[top] > 0).all()
    print(f"rows at a maximum: iterations {out.iterations[top].tolist()} accepted {out.accepted[top].tolist()} stop {out.stop[top].tolist()}")
    check_identities(out, case_ref("flat"), dict(points=c["points"], point_radii=c["radii"]), "flat", c["R"], c["t"])


@pytest.mark.parametrize("n", [1, 3, 4, 5])
def test_the_tail_of_the_last_block(n):
    name = "ref65"
    c = overlay_cases.case(name)
    pick = [int(np.flatnonzero([len(p) == 256 for p in c["points"]])[0]), 2, 12, 5, 0][:n]  # (256 points first: the longest row of the call stands in wave 0)
    out = run(name, rows=pick)
    ref = overlay_cases.reference(name)
    check_against(out, [ref[j] for j in pick], [c["points"][j] for j in pick], f"a call of {n} rows", overlay_cases.bar(name))
    assert same_bits(out, result(name), rows=pick)


def test_same_bits_twice_and_wherever_a_row_stands():
    name = "ref41"
    a = result(name)
    assert same_bits(run(name), a)
    perm = np.random.default_rng(3).permutation(len(a))
    assert same_bits(run(name, rows=perm), a, rows=perm)
    moving = int(np.flatnonzero(a.accepted > 2)[0])
    rows = [moving] + list(range(5)) + [moving] * 3 + list(range(5, 9)) + [moving]  # first, repeated, last
    assert same_bits(run(name, rows=rows), a, rows=rows)


# ---------------------------------------------------------------------------------------------------------------- 2. the start motions
def check_starts(got, want, tag):
    worst = 0.0
    for i, w in enumerate(want):
        assert got.status[i] == w["status"], (tag, i)
        dev = np.concatenate([got.rotation[i].reshape(-1), got.translation[i], got.centre[i], got.axes[i].reshape(-1), got.values[i]])
        ref = np.concatenate([w["rotation"].reshape(-1), w["translation"], w["frame"][:15]])
        if w["status"] != 0:
            assert np.isnan(dev).all(), (tag, i)
            continue
        worst = max(worst, float(np.abs(dev - ref).max()))
        E = got.axes[i].T
        scale = max(float(got.values[i].sum()), 1e-300)
        assert np.abs(E.T @ E - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(E) - 1.0) <= 1e-14, (tag, i)
        assert got.values[i][0] >= got.values[i][1] >= got.values[i][2] >= -1e-10 * scale, (tag, i)
        R = got.rotation[i]
        assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(R) - 1.0) <= 1e-14, (tag, i)
    bits = all(np.array_equal(got.rotation[i], w["rotation"]) and np.array_equal(got.translation[i], w["translation"]) for i, w in enumerate(want) if w["status"] == 0)
    print(f"{tag}: {len(want)} start rows, worst difference from the restatement {worst:.3e} (bar 1e-12), motions bit-equal: {bits}")
    assert worst <= 1e-12, (tag, worst)


@pytest.mark.parametrize("name", ["ref1", "ref41", "ref65", "ref256"])
def test_starts_against_the_restatement(name):
    from pharmaconet_amd.engine import overlay_starts

    c = overlay_cases.case(name)
    start = np.arange(c["n"]) % 4
    start[5], start[9] = 4, -1  # (not a start)
    got = overlay_starts(case_ref(name), start, points=c["points"])
    want = [overlay_ref.starts_row(c["ref_xyz"], c["points"][i], start[i]) for i in range(c["n"])]
    check_starts(got, want, f"starts, {name}")
    assert got.status[5] == got.status[9] == 4 and (np.delete(got.status, [5, 9]) == 0).all()
    d = c["points"][4].astype(np.float64) - got.centre[4]  # the frame diagonalises the row's own scatter
    D = got.axes[4] @ (d.T @ d) @ got.axes[4].T
    assert np.abs(D - np.diag(np.diag(D))).max() <= 1e-10 * np.trace(D) and np.allclose(np.diag(D), got.values[4], rtol=1e-9, atol=1e-10 * np.trace(D))


def test_four_starts_keep_the_best_and_the_lower_among_equals():
    from pharmaconet_amd.engine import overlay, overlay_starts

    xyz, radius = overlay_cases.ligand_6oim()
    rng = np.random.default_rng(11)
    Q = shape_ref.random_rotations(rng, 2)
    centred = xyz.astype(np.float64) - xyz.mean(axis=0)
    bad = np.array([1.5] * 4 + [np.nan], np.float32)
    points = [(centred @ Q[0].T + 7.0).astype(np.float32), np.zeros((0, 3), np.float32), (centred @ Q[1].T - 3.0).astype(np.float32), np.ones((5, 3), np.float32),
              np.array([[1.0, 2.0, 3.0]], np.float32)]
    radii = [radius, np.zeros(0, np.float32), radius, bad, np.array([1.7], np.float32)]
    ref = golden_reference()
    out = overlay(ref, points=points, point_radii=radii, starts=4, max_iter=64, ftol=1e-9)
    print(f"starts=4: kept {out.start.tolist()}, final Tanimoto of every start\n{np.round(out.start_tanimoto, 4)}")
    assert len(out) == 5 and out.start_tanimoto.shape == (5, 4) and out.status.tolist() == [0, 0, 0, 4, 0]
    value = np.where(np.isnan(out.start_tanimoto), -np.inf, out.start_tanimoto)
    assert np.array_equal(out.start, np.argmax(value, axis=1)) and np.array_equal(out.tanimoto[[0, 1, 2, 4]], out.start_tanimoto[np.arange(5), out.start][[0, 1, 2, 4]])
    assert out.tanimoto[0] > 0.999 and out.tanimoto[2] > 0.999 and np.sort(out.start_tanimoto[0])[-2] < 0.95  # a turned copy is found by one start
    assert out.start[1] == 0 and (out.start_tanimoto[1] == 0).all() and out.stop[1] == 0  # no point: four equal starts, the lowest is kept
    assert out.start[3] == 0 and np.isnan(out.start_tanimoto[3]).all() and np.isnan(out.rotation[3]).all() and out.stop[3] == -1
    # each kept row is the overlay of that start's motion, bit for bit
    st = overlay_starts(ref, out.start, points=points)
    ok = [0, 1, 2, 4]
    again = overlay(ref, rotation=st.rotation[ok], translation=st.translation[ok], points=[points[i] for i in ok], point_radii=[radii[i] for i in ok], max_iter=64, ftol=1e-9)
    for f in FIELDS[:14]:
        assert np.array_equal(getattr(again, f), getattr(out, f)[ok]), f
    with pytest.raises(ValueError):
        overlay(ref, points=points, starts=2)
    with pytest.raises(ValueError):
        overlay(ref, points=[points[4]] * 16385, starts=4)


# ---------------------------------------------------------------------------------------------------------------- 3. node mode
def test_node_mode_at_the_first_and_the_last_conformer():
    """The rows are a golden set's ligands at their first and last conformers, started from the restatement's own inertial start 0, so the
    inputs - and every row's decision margin - are known without a GPU."""
    from pharmaconet_amd.engine import overlay, overlay_starts

    model, lib, weights, _ = load_golden("set_6oim_c8")
    ref = golden_reference()
    heads = lib.headers()
    idx = np.arange(min(len(lib), 24))
    o_bb = shape_ref.self_overlap(ref.xyz, ref.radius)
    for which in ("first", "last"):
        conf = np.array([0 if which == "first" else int(heads[int(i), 1]) - 1 for i in idx])
        nodes = [lib.unpack(int(i))["xyz"][:, :, int(c)].astype(np.float32) for i, c in zip(idx, conf)]
        starts = [overlay_ref.starts_row(ref.xyz, nodes[r], 0) for r in range(len(idx))]
        R, t = np.array([s["rotation"] for s in starts]), np.array([s["translation"] for s in starts])
        check_starts(overlay_starts(ref, np.zeros(len(idx), int), library=lib, indices=idx, conformers=conf), starts, f"starts, nodes, {which} conformer")
        refs = {v: [overlay_ref.overlay_row(ref.xyz, ref.radius, nodes[r], np.float32(1.7), R[r], t[r], ftol=FTOL, variant=v, seed=1000 + r, o_bb=o_bb) for r in range(len(idx))]
                for v in ("forward", "reverse", "jitter")}
        s_nodes = variants_apart(refs, nodes)
        print(f"nodes, set_6oim_c8, {which} conformer: S {s_nodes:.3e}")
        out = overlay(ref, library=lib, indices=idx, conformers=conf, rotation=R, translation=t, node_radius=1.7, ftol=FTOL)
        check_against(out, refs["forward"], nodes, f"nodes, {which} conformer", max(1e-12, 1000 * s_nodes))
        check_identities(out, ref, dict(library=lib, indices=idx, conformers=conf, node_radius=1.7), f"nodes, {which}", R, t)
        assert np.array_equal(out.indices, idx) and np.array_equal(out.conformers, conf) and (out.accepted > 0).sum() >= len(idx) // 2
        as_points = overlay(ref, rotation=R, translation=t, points=nodes, node_radius=1.7, ftol=FTOL)
        assert same_bits(as_points, out)  # the same float32 positions as points: the same bits


# ---------------------------------------------------------------------------------------------------------------- 4. the atom store
def test_the_atom_store_equals_host_points_bit_for_bit():
    from pharmaconet_amd.atoms import PackedAtoms
    from pharmaconet_amd.engine import DeviceAtoms, overlay, overlay_starts
    from pharmaconet_amd.pocket import atomic_number_radii

    ref = golden_reference()
    rng = np.random.default_rng(12)
    zs = [np.array([1, 1]), rng.choice([6, 7, 8, 16, 17], size=5), rng.choice([6, 7, 8, 9, 35], size=70)]  # (a record of hydrogens alone: header-only)
    ps = [(rng.uniform(-4, 4, size=(len(z), 2, 3)) + ref.xyz.mean(axis=0)).astype(np.float32) for z in zs]
    edge = PackedAtoms.from_arrays(zs, ps)
    lig, conf = [0, 1, 1, 2, 2, 3, 2], [0, 0, 2, 1, -1, 0, 0]
    R, t = np.array([overlay_cases.rotation_about(rng.normal(size=3), 0.3) for _ in lig]), rng.uniform(-1, 1, size=(len(lig), 3))
    ok = [1, 3, 6]
    host_src = dict(points=[ps[lig[i]][:, conf[i]] for i in ok], point_radii=[atomic_number_radii(zs[lig[i]]) for i in ok])
    host = overlay(ref, rotation=R[ok], translation=t[ok], **host_src)
    dat = DeviceAtoms(edge)
    for source in (edge, dat):
        got = overlay(ref, atoms=source, indices=lig, conformers=conf, rotation=R, translation=t)
        assert got.status.tolist() == [1, 0, 4, 0, 4, 1, 0]
        assert same_bits(host, got, rows=ok) and host.n_points.tolist() == [5, 70, 70] and (host.accepted > 0).all()
        bad = [0, 2, 4, 5]
        assert np.isnan(got.rotation[bad]).all() and np.isnan(got.tanimoto[bad]).all() and (got.stop[bad] == -1).all() and (got.n_points[bad] == 0).all()
        assert np.array_equal(got.indices, lig) and np.array_equal(got.conformers, conf)
        four = overlay(ref, atoms=source, indices=lig, conformers=conf, starts=4)
        assert four.status.tolist() == [1, 0, 4, 0, 4, 1, 0] and np.isnan(four.start_tanimoto[bad]).all() and (four.start[bad] == 0).all()
        host4 = overlay(ref, starts=4, **host_src)
        assert same_bits(host4, four, rows=ok) and np.array_equal(host4.start_tanimoto, four.start_tanimoto[ok])
        st = overlay_starts(ref, [0] * len(lig), atoms=source, indices=lig, conformers=conf)
        assert st.status.tolist() == [1, 0, 4, 0, 4, 1, 0] and np.isnan(st.rotation[bad]).all()
        assert np.array_equal(st.rotation[ok], overlay_starts(ref, [0] * 3, points=host_src["points"]).rotation)
    dat.close()
    o_bb = shape_ref.self_overlap(ref.xyz, ref.radius)
    refs = {v: [overlay_ref.overlay_row(ref.xyz, ref.radius, host_src["points"][k], host_src["point_radii"][k], R[i], t[i], variant=v, seed=k, o_bb=o_bb) for k, i in enumerate(ok)]
            for v in ("forward", "reverse", "jitter")}
    check_against(host, refs["forward"], host_src["points"], "the edge store's rows", max(1e-12, 1000 * variants_apart(refs, host_src["points"])))


# ---------------------------------------------------------------------------------------------------------------- 5. statuses and refusals
def test_rows_that_are_not_ok():
    from pharmaconet_amd.engine import overlay, overlay_starts

    model, lib, weights, _ = load_golden("set_6oim_c8")
    ref = golden_reference()
    C = int(lib.header(0)[1])
    bad_r, bad_t = EYE.copy(), ZERO.copy()
    bad_r[1, 2], bad_t[0] = np.nan, np.inf
    idx, conf = [len(lib), 0, 0, 0, 0, 0, len(lib) + 10**9], [0, C, -1, 0, 0, 0, 0]
    out = overlay(ref, library=lib, indices=idx, conformers=conf, rotation=[EYE, EYE, EYE, bad_r, EYE, EYE, EYE], translation=[ZERO, ZERO, ZERO, ZERO, bad_t, ZERO, ZERO])
    assert out.status.tolist() == [1, 4, 4, 4, 4, 0, 1]
    check_identities(out, ref, dict(library=lib, indices=idx, conformers=conf), "statuses, node mode", [EYE, EYE, EYE, bad_r, EYE, EYE, EYE], [ZERO, ZERO, ZERO, ZERO, bad_t, ZERO, ZERO])
    assert overlay_starts(ref, [0, 0, 0, 3, 4, 0, 0], library=lib, indices=idx, conformers=conf).status.tolist() == [1, 4, 4, 0, 4, 0, 1]
    for radius in (0.0, -1.0):
        nodes = overlay(ref, library=lib, indices=[0, len(lib)], conformers=[0, 0], rotation=[EYE, EYE], translation=[ZERO, ZERO], node_radius=radius)
        assert nodes.status.tolist() == [4, 1] and np.isnan(nodes.rotation).all()
    pts = [np.zeros((3, 3), np.float32), np.ones((2, 3), np.float32), np.zeros((0, 3), np.float32), np.ones((70, 3), np.float32), np.zeros((257, 3), np.float32)]
    radii = [[1.5, np.nan, 1.5], [1.5, 1.5], [], [1.5] * 69 + [0.0], [1.5] * 257]
    pm = overlay(ref, rotation=[EYE] * 5, translation=[ZERO] * 5, points=pts, point_radii=radii)
    assert pm.status.tolist() == [4, 0, 0, 4, 1] and pm.stop.tolist()[2] == 0 and pm.n_points[2] == 0 and pm.tanimoto[2] == 0.0 and pm.self_overlap[2] == 0.0
    assert np.array_equal(pm.rotation[2], EYE) and same_bits(overlay(ref, rotation=[EYE], translation=[ZERO], points=[pts[1]], point_radii=[radii[1]]), pm, rows=[1])
    assert overlay_starts(ref, [0] * 5, points=pts).status.tolist() == [0, 0, 0, 0, 1]
    none = overlay(ref, library=lib, indices=[], conformers=[], rotation=np.zeros((0, 3, 3)), translation=np.zeros((0, 3)))
    assert len(none) == 0 and none.rotation.shape == (0, 3, 3) and len(overlay(ref, rotation=[], translation=[], points=[])) == 0 and len(overlay(ref, points=[], starts=4)) == 0
    assert len(overlay_starts(ref, [], points=[])) == 0


def raw_call(ref, fn="overlay", n=1, lib=None, node=False, pts=False, null=(), radius=1.0, ftol=1e-6, max_iter=32):
    """pmx_shape_overlay / pmx_shape_starts itself with one identity row. The return code, the message and the outputs."""
    import torch

    from pharmaconet_amd import _ffi
    from pharmaconet_amd.engine import device_shape_ref

    dev = torch.device("cuda", torch.cuda.current_device())
    rh = device_shape_ref(ref, dev.index)
    f64 = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)  # noqa: E731
    lig, conf = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    off, xyz = torch.tensor([0, 1], dtype=torch.int64, device=dev), torch.zeros((1, 3), dtype=torch.float32, device=dev)
    rot, trans = f64(np.eye(3).reshape(1, 9)), f64(np.zeros((1, 3)))
    out = dict(rot=torch.full((1, 9), 7.0, dtype=torch.float64, device=dev), trans=torch.full((1, 3), 7.0, dtype=torch.float64, device=dev),
               energy=torch.full((1, 8), 7.0, dtype=torch.float64, device=dev), count=torch.full((1, 4), 7, dtype=torch.int32, device=dev),
               frame=torch.full((1, 16), 7.0, dtype=torch.float64, device=dev), status=torch.full((1,), 7, dtype=torch.int32, device=dev))
    ptr = {k: (None if k in null else v.data_ptr()) for k, v in out.items()}
    stream = torch.cuda.current_stream(dev)
    ffi = _ffi.load()
    src = (lib.handle if node else None, lig.data_ptr() if node else None, conf.data_ptr() if node else None, off.data_ptr() if pts else None, xyz.data_ptr() if pts else None)
    if fn == "overlay":
        rc = ffi.pmx_shape_overlay(rh.handle, *src, None, rot.data_ptr(), trans.data_ptr(), n, radius, ftol, max_iter, ptr["rot"], ptr["trans"], ptr["energy"], ptr["count"],
                                   ptr["status"], ctypes.c_void_p(stream.cuda_stream))
    else:
        rc = ffi.pmx_shape_starts(rh.handle, *src, None if "start" in null else conf.data_ptr(), n, ptr["rot"], ptr["trans"], ptr["frame"], ptr["status"],
                                  ctypes.c_void_p(stream.cuda_stream))
    stream.synchronize()
    return rc, (ffi.pmx_last_error() or b"").decode(), {k: v.cpu().numpy() for k, v in out.items()}


def test_refused_calls():
    from pharmaconet_amd import _ffi
    from pharmaconet_amd.engine import DeviceLibrary, overlay

    model, lib, weights, _ = load_golden("set_6oim_c8")
    ref = golden_reference()
    dlib = DeviceLibrary(lib)
    untouched = lambda out: all((v == 7).all() for v in out.values())  # noqa: E731
    for kw, word in ((dict(lib=dlib, node=True, pts=True), "one source"), (dict(), "neither"), (dict(pts=True, max_iter=65), "max_iter"), (dict(pts=True, max_iter=-1), "max_iter"),
                     (dict(pts=True, ftol=-1.0), "ftol"), (dict(pts=True, ftol=float("nan")), "ftol"), (dict(pts=True, radius=float("inf")), "point_radius"),
                     (dict(pts=True, n=65537), "rows"), (dict(pts=True, n=0, max_iter=65), "max_iter")):
        rc, msg, out = raw_call(ref, **kw)
        assert rc == 1 and msg.startswith("pmx_shape_overlay") and word in msg and untouched(out), (kw, rc, msg)
    for kw, word in ((dict(lib=dlib, node=True, pts=True), "one source"), (dict(), "neither"), (dict(pts=True, n=65537), "rows"), (dict(pts=True, null=("start",)), "start_dev")):
        rc, msg, out = raw_call(ref, fn="starts", **kw)
        assert rc == 1 and msg.startswith("pmx_shape_starts") and word in msg and untouched(out), (kw, rc, msg)
    for fn, names in (("overlay", ("rot", "trans", "energy", "count", "status")), ("starts", ("rot", "trans", "frame", "status"))):
        for name in names:
            for kw in (dict(pts=True), dict(lib=dlib, node=True)):
                rc, msg, out = raw_call(ref, fn=fn, null=(name,), **kw)
                assert rc == 1 and "null output" in msg and untouched(out), (fn, name, kw, msg)
        rc, _, out = raw_call(ref, fn=fn, n=0, pts=True)
        assert rc == 0 and untouched(out)  # n = 0 succeeds and writes nothing
        for kw in (dict(pts=True), dict(lib=dlib, node=True), dict(pts=True, max_iter=64), dict(pts=True, max_iter=0, ftol=0.0)):
            rc, _, out = raw_call(ref, fn=fn, **kw)
            assert rc == 0 and int(out["status"][0]) == 0 and np.isfinite(out["rot"]).all(), (fn, kw)
    lib_ = _ffi.load()
    assert lib_.pmx_shape_overlay(None, *([None] * 8), 0, 1.0, 1e-6, 32, *([None] * 6)) == 1 and b"null reference" in lib_.pmx_last_error()
    assert lib_.pmx_shape_starts(None, *([None] * 6), 0, *([None] * 5)) == 1 and b"null reference" in lib_.pmx_last_error()
    dlib.close()
    eye, zero = [np.eye(3)], [np.zeros(3)]
    for kw in (dict(library=lib, indices=[0], conformers=[0], points=[np.zeros((1, 3))]), dict(), dict(points=[np.zeros((1, 3))], max_iter=65),
               dict(points=[np.zeros((1, 3))], ftol=-1.0), dict(points=[np.zeros((1, 3))], starts=3)):
        with pytest.raises(ValueError):
            overlay(ref, rotation=eye, translation=zero, **kw)
    with pytest.raises(ValueError):
        overlay(ref, points=[np.zeros((1, 3))])  # starts=0 without a motion


# ---------------------------------------------------------------------------------------------------------------- 6. the Python layer
def test_the_python_methods():
    from pharmaconet_amd.engine import overlay
    from test_attribution_cpu import load_mols
    from test_gpu_align import posed
    from test_gpu_clash import pocket_6oim

    model, lib, weights, ex, al = posed("set_6oim_c8")
    mols = load_mols("set_6oim_c8")
    ref = golden_reference()
    pocket = pocket_6oim()
    ok = al.status == 0
    # the local overlay of fitted poses: nodes, and the molecules' atoms
    nodes = al.overlay(ref, lib, node_radius=1.7)
    direct = overlay(ref, library=lib, indices=al.indices, conformers=al.conformers, rotation=al.rotation, translation=al.translation, node_radius=1.7)
    assert same_bits(nodes, direct) and np.array_equal(nodes.indices, al.indices) and np.array_equal(nodes.status == 0, ok)
    check_identities(nodes, ref, dict(library=lib, indices=al.indices, conformers=al.conformers, node_radius=1.7), "Alignment.overlay", al.rotation, al.translation)
    atoms = [mols[int(i)] for i in al.indices]
    ov = al.overlay(ref, atoms=atoms)
    sh0, sh1 = al.shape(ref, atoms=atoms), ov.shape(ref, atoms=atoms)
    assert np.array_equal(ov.tanimoto_start[ok], sh0.tanimoto[ok]) and np.array_equal(ov.overlap[ok], sh1.overlap[ok])
    # (the overlay's Tanimoto keeps the O_AA of the input motion; `shape` at the final one forms its own, which differs by rounding)
    assert np.array_equal(ov.self_overlap[ok], sh0.self_overlap[ok]) and np.allclose(ov.tanimoto[ok], sh1.tanimoto[ok], rtol=1e-12, atol=0)
    assert (ov.tanimoto[ok] >= ov.tanimoto_start[ok]).all() and (ov.accepted[ok] > 0).any() and np.array_equal(ov.indices, al.indices)
    print(f"Alignment.overlay(atoms=), set_6oim_c8: mean Tanimoto {ov.tanimoto_start[ok].mean():.3f} -> {ov.tanimoto[ok].mean():.3f}, median shift {np.median(ov.shift[ok]):.2f} A, "
          f"median angle {np.degrees(np.median(ov.angle[ok])):.1f} deg")
    assert np.array_equal(ov.transform(0, atoms[0].atom_positions[:, 0]), np.asarray(atoms[0].atom_positions[:, 0], dtype=np.float64) @ ov.rotation[0].T + ov.translation[0])
    with pytest.raises(ValueError):
        al.overlay(ref)
    with pytest.raises(ValueError):
        al.overlay(ref, lib, starts=4)
    # the overlaid poses go on through the pose chain
    rep, fit, moved = ov.clashes(pocket, atoms=atoms), ov.pose_fit(model, lib), ov.refine(pocket, atoms=atoms)
    assert np.array_equal(rep.status == 0, ok) and np.array_equal(fit.status == 0, ok) and np.array_equal(moved.status == 0, ok) and np.array_equal(moved.indices, al.indices)
    assert np.array_equal(moved.overlap_start[ok], rep.overlap[ok])
    again = al.refine(pocket, lib).overlay(ref, lib)
    assert np.array_equal(again.status == 0, ok) and (again.overlap[ok] >= again.overlap_start[ok]).all()
    # one ligand
    r = int(np.flatnonzero(ok & (al.n_nodes >= 3))[0])
    i = int(al.indices[r])
    one = model.scoring_overlay(mols[i], ref)
    C = mols[i].atom_positions.shape[1]
    from pharmaconet_amd.engine import _heavy_atoms

    points, radii = _heavy_atoms([mols[i]] * C, range(C))
    every = overlay(ref, points=points, point_radii=radii, starts=4)
    best = int(np.argmax(every.tanimoto))
    assert one["level"] == "atoms" and one["status"] == 0 and one["conformer"] == best and one["start"] == every.start[best] and one["tanimoto"] == every.tanimoto[best]
    assert np.array_equal(one["rotation"], every.rotation[best]) and one["positions"].shape == (mols[i].atom_positions.shape[0], 3)
    local = model.scoring_overlay(mols[i], ref, starts=0, weights=weights)
    assert local["conformer"] == al.conformers[r] and local["start"] == -1 and local["tanimoto"] == ov.tanimoto[r] and np.array_equal(local["rotation"], ov.rotation[r])
    packed = model.scoring_overlay(lib.record(i), ref, level="nodes")
    assert packed["level"] == "nodes" and packed["positions"] is None and packed["status"] == 0 and packed["node_positions"].shape[1] == 3
    with pytest.raises(ValueError):
        model.scoring_overlay(lib.record(i), ref)  # atoms of a packed record
    # the screen's best hits
    small = lib.select(np.arange(24))
    res = model.screen(small, weights=weights)
    top = res.overlay(6, ref, node_radius=1.7)
    hits = res._best(6).astype(np.int64)
    assert len(top) == len(hits) and np.array_equal(top.indices, hits) and top.start_tanimoto.shape == (len(hits), 4) and (top.status == 0).all()
    all_c = res.overlay(6, ref, conformers="all", node_radius=1.7)
    assert np.array_equal(all_c.indices, hits) and (all_c.tanimoto >= top.tanimoto).all()
    heads = small.headers()
    for h, hit in enumerate(hits):
        C = int(heads[hit, 1])
        each = overlay(ref, library=small, indices=[hit] * C, conformers=range(C), starts=4, node_radius=1.7)
        k = int(np.argmax(each.tanimoto))
        assert all_c.conformers[h] == k and all_c.tanimoto[h] == each.tanimoto[k] and all_c.start[h] == each.start[k]
    fitted = res.overlay(6, ref, starts=0, node_radius=1.7)
    assert np.array_equal(fitted.indices, hits) and (fitted.start == -1).all()
    for kw in (dict(conformers="all", starts=0), dict(conformers="some"), dict(starts=2)):
        with pytest.raises(ValueError):
            res.overlay(6, ref, **kw)
    with pytest.raises(ValueError, match="ScreeningResult.overlay"):
        res.overlay(16385, ref)


def test_cli_overlay_csv(tmp_path):
    from pharmaconet_amd.engine import explain, overlay
    from pharmaconet_amd.screening import OVERLAY_HEADER, main

    model, lib, _, _ = load_golden("set_6oim_c8")
    ref = golden_reference()
    lib = lib.select(np.arange(16))
    libfile = tmp_path / "lib.pmxlib"
    lib.save(libfile)
    refpdb = str(GOLDEN / "ligand_6oim_mov.pdb")
    args = ["-p", str(GOLDEN / "model_6oim_like.pm"), "-d", str(libfile), "--explain", "5", "--shape_level", "nodes"]
    main(args + ["-o", str(tmp_path / "plain.csv"), "--explain_out", str(tmp_path / "plain_hits.csv"), "--pose_shape", str(tmp_path / "plain_shape.csv"), "--shape_ref", refpdb])
    main(args + ["-o", str(tmp_path / "with.csv"), "--explain_out", str(tmp_path / "hits.csv"), "--pose_shape", str(tmp_path / "shape.csv"), "--shape_ref", refpdb,
                 "--overlay_out", str(tmp_path / "overlay4.csv"), "--overlay_iter", "16"])
    for a, b in (("plain.csv", "with.csv"), ("plain_hits.csv", "hits.csv"), ("plain_shape.csv", "shape.csv")):
        assert (tmp_path / a).read_bytes() == (tmp_path / b).read_bytes()
    main(args + ["-o", str(tmp_path / "x.csv"), "--overlay_out", str(tmp_path / "overlay0.csv"), "--shape_ref", refpdb, "--overlay_starts", "0"])  # (--shape_ref without --pose_shape)
    base = ["-p", str(GOLDEN / "model_6oim_like.pm"), "-d", str(libfile), "-o", str(tmp_path / "y.csv")]
    for bad in (["--overlay_out", str(tmp_path / "o.csv"), "--shape_ref", refpdb, "--shape_level", "nodes"],  # no --explain
                ["--explain", "5", "--overlay_out", str(tmp_path / "o.csv"), "--shape_level", "nodes"],  # no reference
                ["--explain", "5", "--shape_ref", refpdb],  # a reference for nothing
                ["--explain", "5", "--overlay_out", str(tmp_path / "o.csv"), "--shape_ref", refpdb],  # atoms of a packed library
                ["--explain", "5", "--overlay_out", str(tmp_path / "o.csv"), "--shape_ref", refpdb, "--shape_level", "nodes", "--overlay_iter", "65"],
                ["--explain", "5", "--overlay_out", str(tmp_path / "o.csv"), "--shape_ref", refpdb, "--shape_level", "nodes", "--overlay_starts", "2"]):
        with pytest.raises(SystemExit):
            main(base + bad)
    hits = [row.split(",") for row in (tmp_path / "hits.csv").read_text().splitlines()[1:]]
    names = {f"{libfile}#{i}": i for i in range(len(lib))}
    al = explain(model, lib, [names[h[1]] for h in hits]).poses(model, lib)  # (the command line's default weights are the engine's)
    want = {"overlay4.csv": overlay(ref, library=lib, indices=al.indices, conformers=al.conformers, starts=4, max_iter=16), "overlay0.csv": al.overlay(ref, lib)}
    for name, ov in want.items():
        rows = (tmp_path / name).read_text().splitlines()
        assert rows[0] == OVERLAY_HEADER == ("rank,path,conformer,level,start,points,iterations,stop,tanimoto_start,tanimoto,overlap,reference_fraction,fit_fraction,angle_deg,shift,"
                                             "r00,r01,r02,r10,r11,r12,r20,r21,r22,tx,ty,tz")
        assert len(rows) == len(hits) + 1 == 6
        for r, row in enumerate(rows[1:]):
            f = row.split(",")
            assert len(f) == 27 and int(f[0]) == r + 1 and f[1] == hits[r][1] and int(f[2]) == int(al.conformers[r]) and f[3] == "nodes", (name, r)
            assert [int(v) for v in f[4:8]] == [ov.start[r], ov.n_points[r], ov.iterations[r], ov.stop[r]], (name, r)
            assert float(f[8]) == ov.tanimoto_start[r] and float(f[9]) == ov.tanimoto[r] and repr(float(f[9])) == f[9] and float(f[10]) == ov.overlap[r]
            assert float(f[11]) == ov.overlap[r] / ov.reference_overlap[r] and float(f[12]) == ov.overlap[r] / ov.self_overlap[r]
            assert float(f[13]) == float(np.degrees(ov.angle[r])) and float(f[14]) == ov.shift[r]
            assert np.array_equal(np.array([float(v) for v in f[15:24]]).reshape(3, 3), ov.rotation[r]) and np.array_equal(np.array([float(v) for v in f[24:27]]), ov.translation[r])
