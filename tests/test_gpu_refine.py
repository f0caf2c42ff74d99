"""`pmx_pose_refine` on the GPU (csrc/pmx_refine.hip) against the NumPy restatement of tests/refine_ref.py over the seeded rows of
tests/refine_cases.py: point mode over the point, pocket and anchor counts at which the kernel's trips change, node mode on a golden set's
own poses, the identities with `pmx_pose_clash` that must hold bit for bit, repeatability, statuses, and the Python layer on top of it.

Bars. Integers (status, iterations, accepted steps, stop reason, clashing pairs) must be equal; they can only differ where a row stands
within rounding of a decision, so they are asserted after the restatement's `decision_margin` is at least 1e-9 on every row (the seeds are
chosen so, checked on the CPU by tests/test_refine_cpu.py). Floats: the posed points under the returned motion and the relative final E are
within max(1e-12, 1000 S), S = refine_cases.S[case] being how far rounding alone moves the restatement over the very rows of the case; the factor covers what
its variants do not model one by one - contracted multiply-adds in H and g, the device's sin and cos, division."""

import ctypes
from functools import lru_cache

import numpy as np
import pytest

import clash_ref
import refine_cases
import refine_ref
from conftest import GOLDEN, load_golden
from refine_cases import FTOL, MARGIN, NODE_RADIUS, RESTRAINT, TOLERANCE

pytestmark = pytest.mark.gpu


@lru_cache(maxsize=None)
def case_pocket(name):
    from pharmaconet_amd.pocket import PocketAtoms

    c = refine_cases.case(name)
    return PocketAtoms.from_arrays(c["atom_xyz"], c["atom_radius"], c["atom_group"])


def run(name, rows=None, **kw):
    from pharmaconet_amd.engine import refine

    c = refine_cases.case(name)
    rows = list(range(c["n"])) if rows is None else list(rows)
    pick = lambda v: None if v is None else [v[i] for i in rows]  # noqa: E731
    args = dict(node_radius=NODE_RADIUS, tolerance=TOLERANCE, restraint=RESTRAINT, ftol=FTOL, max_iter=c["max_iter"])
    args.update(kw)
    return refine(case_pocket(name), rotation=c["R"][rows], translation=c["t"][rows], points=pick(c["points"]), point_radii=pick(c["radii"]), anchors=pick(c["anchors"]),
                  anchor_targets=pick(c["targets"]), anchor_weights=pick(c["weights"]), **args)


@lru_cache(maxsize=None)
def result(name):
    return run(name)


FIELDS = ("rotation", "translation", "overlap_start", "overlap", "restraint_start", "restraint_energy", "anchor_rmsd", "angle", "shift", "iterations", "accepted", "stop",
          "n_pairs", "status")


def same_bits(a, b, rows=None):
    rows = np.arange(len(b)) if rows is None else np.asarray(rows)
    return len(a) == len(rows) and all(np.array_equal(getattr(a, f), getattr(b, f)[rows], equal_nan=True) for f in FIELDS)


def check_against(out, ref, points, tag, restraint=RESTRAINT, bar=None):
    """Every row of `out` against the restatement's rows; the figures are printed before they are asserted."""
    assert len(out) == len(ref), tag
    bar = refine_cases.bar(tag) if bar is None else bar
    margin = min([r["decision_margin"] for r in ref], default=np.inf)
    worst_p = worst_e = 0.0
    for i, r in enumerate(ref):
        if r["status"] != 0 or out.status[i] != 0:
            continue
        if len(points[i]):
            worst_p = max(worst_p, float(np.abs(clash_ref.pose(points[i], out.rotation[i], out.translation[i]) - clash_ref.pose(points[i], r["rotation"], r["translation"])).max()))
        E = r["energy"][2] + restraint * r["energy"][3]
        if E > 0:
            worst_e = max(worst_e, abs((out.overlap[i] + restraint * out.restraint_energy[i]) - E) / E)
    print(f"{tag}: rows {len(ref)} decision margin {margin:.3e} worst posed point error {worst_p:.3e} A, worst relative E error {worst_e:.3e} (bar {bar:.1e})")
    assert margin >= MARGIN, (tag, margin)
    for i, r in enumerate(ref):
        got = [int(out.status[i]), int(out.iterations[i]), int(out.accepted[i]), int(out.stop[i]), int(out.n_pairs[i])]
        assert got == [int(r["status"])] + [int(v) for v in r["count"]], (tag, i, got, r["count"])
    assert worst_p <= bar and worst_e <= bar, (tag, worst_p, worst_e, bar)
    # the other floats, loosely: they are functions of the motion and the energies checked above
    for i, r in enumerate(ref):
        if r["status"] == 0:
            got = np.array([out.overlap_start[i], out.restraint_start[i], out.overlap[i], out.restraint_energy[i], out.anchor_rmsd[i], out.angle[i], out.shift[i]])
            assert np.allclose(got, r["energy"][:7], rtol=1e-6, atol=1e-7), (tag, i, got, r["energy"])


def check_identities(out, pocket, source, tag, start_R, start_t, **kw):
    """What must hold bit for bit against `pmx_pose_clash`, and the properties of every OK row."""
    from pharmaconet_amd.engine import clashes

    ok = out.status == 0
    before = clashes(pocket, rotation=start_R, translation=start_t, **source, **kw)
    after = clashes(pocket, rotation=np.where(ok[:, None, None], out.rotation, 0.0), translation=np.where(ok[:, None], out.translation, 0.0), **source, **kw)
    assert np.array_equal(before.status == 0, ok), tag
    assert np.array_equal(out.overlap_start[ok], before.overlap[ok]), tag
    assert np.array_equal(out.overlap[ok], after.overlap[ok]) and np.array_equal(out.n_pairs[ok], after.n_pairs[ok]), tag
    clean = ok & (before.n_pairs == 0)
    assert (out.stop[clean] == 0).all() and (out.iterations[clean] == 0).all() and (out.stop[ok & ~clean] > 0).all(), tag
    same = ok & (out.accepted == 0)
    assert clean[ok].sum() == (out.stop[ok] == 0).sum() and (same | ~clean).all(), tag
    assert np.array_equal(out.rotation[same], np.asarray(start_R)[same]) and np.array_equal(out.translation[same], np.asarray(start_t)[same]), tag
    assert (out.angle[same] == 0).all() and (out.shift[same] == 0).all(), tag
    return before, after


def check_properties(out, restraint, start_R, tag):
    ok = out.status == 0
    E0, E1 = out.overlap_start + restraint * out.restraint_start, out.overlap + restraint * out.restraint_energy
    assert (E1[ok] <= E0[ok]).all() and (E1[ok & (out.accepted > 0)] < E0[ok & (out.accepted > 0)]).all(), tag
    R, R0 = out.rotation[ok], np.asarray(start_R)[ok]
    square = np.abs(np.einsum("nji,njk->nik", R0, R0) - np.eye(3)).reshape(len(R0), -1).max(axis=1, initial=0.0) <= 1e-15  # (the inputs that are orthogonal to 1e-15)
    assert square.sum() >= len(R0) // 2, tag
    assert np.abs(np.einsum("nji,njk->nik", R[square], R[square]) - np.eye(3)).max(initial=0.0) <= 1e-13 and (np.linalg.det(R) > 0).all(), tag
    bad = ~ok
    assert np.isnan(out.rotation[bad]).all() and np.isnan(out.translation[bad]).all() and (out.stop[bad] == -1).all() and (out.iterations[bad] == 0).all(), tag
    for f in ("overlap_start", "overlap", "restraint_start", "restraint_energy", "anchor_rmsd", "angle", "shift"):
        assert np.isnan(getattr(out, f)[bad]).all() and np.isfinite(getattr(out, f)[ok]).all(), (tag, f)


# ---------------------------------------------------------------------------------------------------------------- 1. point mode, every case
@pytest.mark.parametrize("name", list(refine_cases.CASES))
def test_point_mode_against_the_restatement(name):
    c = refine_cases.case(name)
    out = result(name)
    check_against(out, refine_cases.reference(name), c["points"], name)
    source = dict(points=c["points"], point_radii=c["radii"], node_radius=NODE_RADIUS)
    check_identities(out, case_pocket(name), source, name, c["R"], c["t"], tolerance=TOLERANCE)
    check_properties(out, RESTRAINT, c["R"], name)
    if c["max_iter"] == 0:
        assert np.array_equal(out.rotation, c["R"]) and np.array_equal(out.translation, c["t"]) and set(out.stop.tolist()) == {0, 2}
    if len(c["atom_xyz"]) == 0:
        assert (out.stop == 0).all()
    else:
        assert (out.accepted > 0).any() or c["max_iter"] == 0
    assert {len(p) for p in c["points"]} == set(refine_cases.COUNTS)
    if c["anchors"] is not None:
        assert {len(a) for a in c["anchors"]} == set(refine_cases.ANCHOR_COUNTS)


# ---------------------------------------------------------------------------------------------------------------- 2. node mode
def pocket_6oim():
    from test_gpu_clash import pocket_6oim as cached

    return cached()


NODE_FTOL = 1e-5


def test_node_mode_on_a_golden_sets_own_poses():
    """The rows are the set's own poses as `pmx_align` fits them on the GPU, so there is no seed to choose and nothing to work out without
    a GPU. ftol is fixed instead: at 1e-5 the restatement, run from those motions, has every row 7.1e-8 or more from a decision (at 1e-6 one
    row stands 1.0e-11 from one; at the default 1e-9 a converged row stands within 1e-9 of its last by construction: tests/refine_cases.py).
    The bar is made as for the seeded cases, from the restatement's three variants over these very rows."""
    from pharmaconet_amd.engine import refine
    from test_gpu_align import posed

    model, lib, weights, ex, al = posed("set_6oim_c8")
    pocket = pocket_6oim()
    nodes = [lib.unpack(int(i))["xyz"][:, :, int(c)].astype(np.float32) for i, c in zip(al.indices, al.conformers)]
    refs = {v: [refine_ref.refine_row(pocket.xyz, pocket.radius, nodes[r], np.float32(1.0), al.rotation[r], al.translation[r], ftol=NODE_FTOL, variant=v, seed=1000 + r)
                for r in range(len(al))] for v in ("forward", "reverse", "jitter")}
    ref = refs["forward"]
    s_nodes = 0.0
    for r in range(len(al)):
        for v in ("reverse", "jitter"):
            other = refs[v][r]
            assert other["status"] == ref[r]["status"] and np.array_equal(other["count"], ref[r]["count"]) and other["decision_margin"] >= MARGIN, (r, v)
            if ref[r]["status"] == 0:
                s_nodes = max(s_nodes, float(np.abs(clash_ref.pose(nodes[r], other["rotation"], other["translation"]) - clash_ref.pose(nodes[r], ref[r]["rotation"], ref[r]["translation"])).max(initial=0.0)))
                E = [x["energy"][2] + 0.1 * x["energy"][3] for x in (ref[r], other)]
                s_nodes = max(s_nodes, abs(E[1] - E[0]) / E[0] if E[0] > 0 else 0.0)
    print(f"nodes, set_6oim_c8: S {s_nodes:.3e}")
    out = al.refine(pocket, lib, ftol=NODE_FTOL)
    assert len(out) == len(al) and np.array_equal(out.indices, al.indices) and np.array_equal(out.conformers, al.conformers) and np.array_equal(out.status == 0, al.status == 0)
    check_against(out, ref, nodes, "nodes, set_6oim_c8", bar=max(1e-12, 1000 * s_nodes))
    before, after = check_identities(out, pocket, dict(library=lib, indices=al.indices, conformers=al.conformers), "nodes", al.rotation, al.translation)
    check_properties(out, 0.1, al.rotation, "nodes")
    assert (out.accepted > 0).any()  # the model is in the crystal frame: some fitted poses graze the protein
    # the same float32 positions as points, and as explicit anchors: the same bits
    as_points = refine(pocket, rotation=al.rotation, translation=al.translation, points=nodes, node_radius=1.0, ftol=NODE_FTOL)
    as_anchors = refine(pocket, rotation=al.rotation, translation=al.translation, points=nodes, anchors=nodes, node_radius=1.0, ftol=NODE_FTOL)
    assert same_bits(as_points, out) and same_bits(as_anchors, out)
    # Alignment.refine(...).clashes(...) is the check at the refined motion
    rep = out.clashes(pocket, lib)
    ok = out.status == 0
    assert np.array_equal(rep.overlap[ok], out.overlap[ok]) and np.array_equal(rep.n_pairs[ok], out.n_pairs[ok]) and np.array_equal(rep.status, out.status)
    assert np.array_equal(rep.overlap[ok], after.overlap[ok]) and np.isnan(rep.overlap[~ok]).all()
    moved = (before.ok() != rep.ok()).sum()
    print(f"nodes, set_6oim_c8: {int((~before.ok() & ok).sum())} of {int(ok.sum())} poses fail the check, {int((~before.ok() & rep.ok()).sum())} of them pass after the refinement "
          f"({int(moved)} changed); anchor rmsd of the refined rows: median {np.median(out.anchor_rmsd[ok & (out.accepted > 0)]):.3f} A")


# ---------------------------------------------------------------------------------------------------------------- 3. repeatability
def test_same_bits_twice_and_wherever_a_row_stands():
    name = "anchors_tw"
    a = result(name)
    assert same_bits(run(name), a)
    n = len(a)
    perm = np.random.default_rng(3).permutation(n)
    assert same_bits(run(name, rows=perm), a, rows=perm)
    moving = int(np.flatnonzero(a.accepted > 2)[0])
    rows = [moving] + list(range(5)) + [moving] * 3 + list(range(5, 9)) + [moving]  # first, repeated, last
    assert same_bits(run(name, rows=rows), a, rows=rows)


# ---------------------------------------------------------------------------------------------------------------- 4. statuses
def test_statuses():
    from pharmaconet_amd.engine import refine

    model, lib, weights, _ = load_golden("set_6oim_c8")
    pocket = pocket_6oim()
    C = int(lib.header(0)[1])
    eye, zero = np.eye(3), np.zeros(3)
    bad_r, bad_t = eye.copy(), zero.copy()
    bad_r[1, 2], bad_t[0] = np.nan, np.inf
    out = refine(pocket, library=lib, indices=[len(lib), 0, 0, 0, 0, 0, len(lib) + 10**9], conformers=[0, C, -1, 0, 0, 0, 0], rotation=[eye, eye, eye, bad_r, eye, eye, eye],
                 translation=[zero, zero, zero, zero, bad_t, zero, zero])
    assert out.status.tolist() == [1, 4, 4, 4, 4, 0, 1]
    check_properties(out, 0.1, [eye] * 7, "statuses, node mode")
    pts = [np.zeros((3, 3)), np.zeros((2, 3)), np.zeros((2, 3)), np.zeros((2, 3)), np.zeros((2, 3))]
    anchors = [np.zeros((1, 3))] * 5
    pm = refine(pocket, rotation=[bad_r, eye, eye, eye, eye], translation=[zero] * 5, points=pts, anchors=anchors, anchor_weights=[[1.0], [-1e-300], [np.nan], [np.inf], [0.0]])
    assert pm.status.tolist() == [4, 4, 4, 4, 0]
    check_properties(pm, 0.1, [eye] * 5, "statuses, point mode")
    assert (pm.n_pairs[:4] == 0).all() and (pm.accepted[:4] == 0).all() and pm.anchor_rmsd[4] == 0.0  # (no weight: an rmsd of 0)
    empty = refine(pocket, rotation=np.zeros((0, 3, 3)), translation=np.zeros((0, 3)), points=[])
    assert len(empty) == 0 and empty.rotation.shape == (0, 3, 3) and len(refine(pocket, library=lib, indices=[], conformers=[], rotation=[], translation=[])) == 0


# ---------------------------------------------------------------------------------------------------------------- 5. refused calls
def raw_call(pocket, n=1, lib=None, node=False, pts=False, null=(), restraint=0.1, ftol=1e-9, max_iter=32, anchors=(True, True)):
    """pmx_pose_refine itself with one identity row. The return code and the message."""
    import torch

    from pharmaconet_amd import _ffi
    from pharmaconet_amd.engine import device_pocket

    dev = torch.device("cuda", torch.cuda.current_device())
    ph = device_pocket(pocket, dev.index)
    f64 = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)  # noqa: E731
    lig, conf = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    off, xyz = torch.tensor([0, 1], dtype=torch.int64, device=dev), torch.zeros((1, 3), dtype=torch.float32, device=dev)
    rot, trans = f64(np.eye(3).reshape(1, 9)), f64(np.zeros((1, 3)))
    out = dict(rot=torch.empty((1, 9), dtype=torch.float64, device=dev), trans=torch.empty((1, 3), dtype=torch.float64, device=dev),
               energy=torch.empty((1, 8), dtype=torch.float64, device=dev), count=torch.empty((1, 4), dtype=torch.int32, device=dev),
               status=torch.empty(1, dtype=torch.int32, device=dev))
    ptr = {k: (None if k in null else v.data_ptr()) for k, v in out.items()}
    stream = torch.cuda.current_stream(dev)
    ffi = _ffi.load()
    rc = ffi.pmx_pose_refine(ph.handle, lib.handle if node else None, lig.data_ptr() if node else None, conf.data_ptr() if node else None, off.data_ptr() if pts else None,
                             xyz.data_ptr() if pts else None, None, off.data_ptr() if anchors[0] else None, xyz.data_ptr() if anchors[1] else None, None, None,
                             rot.data_ptr(), trans.data_ptr(), n, 1.0, 0.5, restraint, ftol, max_iter, ptr["rot"], ptr["trans"], ptr["energy"], ptr["count"], ptr["status"],
                             ctypes.c_void_p(stream.cuda_stream))
    stream.synchronize()
    return rc, (ffi.pmx_last_error() or b"").decode(), out


def test_refused_calls():
    from pharmaconet_amd.engine import DeviceLibrary, refine

    model, lib, weights, _ = load_golden("set_6oim_c8")
    pocket = pocket_6oim()
    dlib = DeviceLibrary(lib)
    for kw, word in ((dict(lib=dlib, node=True, pts=True), "one source"), (dict(), "neither"), (dict(pts=True, max_iter=65), "max_iter"), (dict(pts=True, max_iter=-1), "max_iter"),
                     (dict(pts=True, restraint=-0.5), "restraint"), (dict(pts=True, restraint=float("nan")), "restraint"), (dict(pts=True, ftol=-1.0), "ftol"),
                     (dict(pts=True, ftol=float("inf")), "ftol"), (dict(pts=True, n=65537), "rows"), (dict(pts=True, anchors=(True, False)), "anchor"),
                     (dict(pts=True, n=0, max_iter=65), "max_iter")):
        rc, msg, _ = raw_call(pocket, **kw)
        assert rc == 1 and msg.startswith("pmx_pose_refine") and word in msg, (kw, rc, msg)
    for name in ("rot", "trans", "energy", "count", "status"):
        for kw in (dict(pts=True), dict(lib=dlib, node=True)):
            rc, msg, _ = raw_call(pocket, null=(name,), **kw)
            assert rc == 1 and "null output" in msg, (name, kw, msg)
    assert raw_call(pocket, n=0, pts=True)[0] == 0
    for kw in (dict(pts=True), dict(lib=dlib, node=True), dict(pts=True, anchors=(False, False)), dict(pts=True, max_iter=64), dict(pts=True, max_iter=0, restraint=0.0, ftol=0.0)):
        rc, _, out = raw_call(pocket, **kw)
        assert rc == 0 and int(out["status"].cpu()[0]) == 0 and int(out["count"].cpu()[0, 2]) >= 0 and np.isfinite(out["rot"].cpu().numpy()).all(), kw
    dlib.close()
    eye, zero = [np.eye(3)], [np.zeros(3)]
    for kw in (dict(library=lib, indices=[0], conformers=[0], points=[np.zeros((1, 3))]), dict(), dict(points=[np.zeros((1, 3))], max_iter=65),
               dict(points=[np.zeros((1, 3))], restraint=-1.0), dict(points=[np.zeros((1, 3))], anchor_weights=[[1.0]]),
               dict(points=[np.zeros((1, 3))], anchors=[np.zeros((2, 3))], anchor_weights=[[1.0]])):
        with pytest.raises(ValueError):
            refine(pocket, rotation=eye, translation=zero, **kw)


# ---------------------------------------------------------------------------------------------------------------- 6. the Python layer
def test_alignment_refine_with_atoms_and_scoring_refine():
    from pharmaconet_amd.engine import _heavy_atoms
    from test_attribution_cpu import load_mols
    from test_gpu_align import posed

    model, lib, weights, ex, al = posed("set_6oim_c8")
    mols = load_mols("set_6oim_c8")
    pocket = pocket_6oim()
    atoms = [mols[int(i)] for i in al.indices]
    out = al.refine(pocket, atoms=atoms)
    points, radii = _heavy_atoms(atoms, al.conformers)
    check_identities(out, pocket, dict(points=points, point_radii=radii), "Alignment.refine(atoms=)", al.rotation, al.translation)
    check_properties(out, 0.1, al.rotation, "Alignment.refine(atoms=)")
    rep = out.clashes(pocket, atoms=atoms)
    ok = out.status == 0
    assert np.array_equal(rep.overlap[ok], out.overlap[ok]) and np.array_equal(rep.n_pairs[ok], out.n_pairs[ok]) and (out.accepted > 0).any()
    assert np.array_equal(out.transform(0, points[0]), points[0].astype(np.float64) @ out.rotation[0].T + out.translation[0])
    with pytest.raises(ValueError):
        al.refine(pocket)
    # one ligand
    r = next(r for r in range(len(al)) if al.n_nodes[r] >= 3)
    i = int(al.indices[r])
    one = model.scoring_refine(mols[i], weights=weights, pocket=pocket)
    assert one["level"] == "atoms" and one["status"] == 0 and one["conformer"] == al.conformers[r] and np.array_equal(one["rotation"], al.rotation[r])
    assert np.array_equal(one["refined_rotation"], out.rotation[r]) and np.array_equal(one["refined_translation"], out.translation[r])
    assert (one["overlap_start"], one["overlap"], one["anchor_rmsd"], one["iterations"], one["stop"], one["n_pairs"]) == (
        out.overlap_start[r], out.overlap[r], out.anchor_rmsd[r], out.iterations[r], out.stop[r], out.n_pairs[r]) and one["ok"] == bool(rep.ok()[r])
    nodes = al.refine(pocket, lib)
    packed = model.scoring_refine(lib.record(i), weights=weights, pocket=pocket)
    assert packed["level"] == "nodes" and packed["overlap"] == nodes.overlap[r] and packed["iterations"] == nodes.iterations[r]


def test_fitting_with_and_without_refinement():
    import dataclasses

    from test_gpu_clash import same_bits as same_report

    model, lib, weights, _ = load_golden("set_6oim_c8")
    pocket = pocket_6oim()
    lib = lib.select(np.arange(24))
    res = model.screen(lib, weights=weights)
    for max_clashing in (0, 2):
        plain = res.fitting(16, pool=16, max_clashing=max_clashing, pocket=pocket)
        off = res.fitting(16, pool=16, max_clashing=max_clashing, pocket=pocket, refine=False) if max_clashing == 0 else plain
        assert plain.refined is None and off.refined is None
        for f in dataclasses.fields(plain):
            a, b = getattr(plain, f.name), getattr(off, f.name)
            if f.name == "report":
                assert same_report(a, b)
            elif f.name == "poses":
                assert np.array_equal(a.rotation, b.rotation, equal_nan=True) and np.array_equal(a.translation, b.translation, equal_nan=True) and np.array_equal(a.status, b.status)
            elif f.name != "refined":
                assert np.array_equal(a, b), f.name
        # a smaller tolerance for the refinement than for the check: a penalty balanced against a restraint leaves a little overlap
        fit = res.fitting(16, pool=16, max_clashing=max_clashing, pocket=pocket, refine=True, refine_tolerance=0.0)
        failing = ~plain.report.ok(max_clashing) & (plain.poses.status == 0)
        assert set(plain.rows.tolist()) <= set(fit.rows.tolist()) and len(fit) >= len(plain)
        assert (fit.refined is not None) == bool(failing.any()) and np.array_equal(fit.pool, plain.pool)
        passes = fit.report.ok(max_clashing) & (fit.poses.status == 0)
        assert np.array_equal(fit.rows, np.flatnonzero(passes)[:16]) and np.array_equal(fit.indices, fit.poses.indices[fit.rows].astype(np.uint64))
        if fit.refined is not None:
            used = failing & (fit.refined.status == 0)
            assert np.array_equal(fit.poses.rotation[used], fit.refined.rotation[used]) and np.array_equal(fit.poses.rotation[~used], plain.poses.rotation[~used], equal_nan=True)
            assert np.array_equal(fit.report.overlap[~used], plain.report.overlap[~used], equal_nan=True)
            again = fit.poses.clashes(pocket, lib)
            assert np.array_equal(again.overlap, fit.report.overlap, equal_nan=True) and np.array_equal(again.n_clashing, fit.report.n_clashing)
        print(f"fitting, max_clashing {max_clashing}: {len(plain)} of 16 pass, {len(fit)} with the refinement at tolerance 0")
    with pytest.raises(ValueError):
        res.fitting(5, pocket=pocket, restraint=0.5)  # (an argument of the refinement, which is off)


def test_cli_refine_csv(tmp_path):
    from pharmaconet_amd.engine import explain
    from pharmaconet_amd.screening import REFINE_HEADER, main

    model, lib, _, _ = load_golden("set_6oim_c8")
    pocket = pocket_6oim()
    lib = lib.select(np.arange(16))
    libfile = tmp_path / "lib.pmxlib"
    lib.save(libfile)
    args = ["-p", str(GOLDEN / "model_6oim_like.pm"), "-d", str(libfile), "--explain", "5", "--protein", str(GOLDEN / "pocket_6oim.pdb"), "--clash_level", "nodes"]
    main(args + ["-o", str(tmp_path / "plain.csv"), "--explain_out", str(tmp_path / "plain_hits.csv"), "--clashes", str(tmp_path / "plain_clashes.csv")])
    main(args + ["-o", str(tmp_path / "with.csv"), "--explain_out", str(tmp_path / "hits.csv"), "--clashes", str(tmp_path / "clashes.csv"), "--refine_out", str(tmp_path / "refine.csv"),
                 "--refine_restraint", "0.2", "--refine_iter", "16"])
    for a, b in (("plain.csv", "with.csv"), ("plain_hits.csv", "hits.csv"), ("plain_clashes.csv", "clashes.csv")):
        assert (tmp_path / a).read_bytes() == (tmp_path / b).read_bytes()
    base = ["-p", str(GOLDEN / "model_6oim_like.pm"), "-d", str(libfile), "-o", str(tmp_path / "x.csv"), "--protein", str(GOLDEN / "pocket_6oim.pdb")]
    for bad in (["--refine_out", str(tmp_path / "r.csv"), "--clash_level", "nodes"],  # no --explain
                ["--explain", "5", "--refine_out", str(tmp_path / "r.csv")],  # atoms of a packed library
                ["--explain", "5", "--refine_out", str(tmp_path / "r.csv"), "--clash_level", "nodes", "--refine_iter", "65"],
                ["--explain", "5", "--refine_out", str(tmp_path / "r.csv"), "--clash_level", "nodes", "--refine_restraint", "-1"]):
        with pytest.raises(SystemExit):
            main(base + bad)
    hits = [row.split(",") for row in (tmp_path / "hits.csv").read_text().splitlines()[1:]]
    clash_rows = [row.split(",") for row in (tmp_path / "clashes.csv").read_text().splitlines()[1:]]
    rows = (tmp_path / "refine.csv").read_text().splitlines()
    assert rows[0] == REFINE_HEADER == ("rank,path,conformer,level,pairs_before,overlap_before,pairs_after,overlap_after,clearance_after,clashing_after,anchor_rmsd,angle_deg,"
                                        "shift,iterations,stop,r00,r01,r02,r10,r11,r12,r20,r21,r22,tx,ty,tz")
    assert len(rows) == len(hits) + 1 == 6
    names = {f"{libfile}#{i}": i for i in range(len(lib))}
    al = explain(model, lib, [names[h[1]] for h in hits]).poses(model, lib)  # (the command line's default weights are the engine's)
    ref = al.refine(pocket, lib, restraint=0.2, max_iter=16)
    rep = ref.clashes(pocket, lib)
    for r, row in enumerate(rows[1:]):
        f = row.split(",")
        assert len(f) == 27 and int(f[0]) == r + 1 and f[1] == hits[r][1] and int(f[2]) == int(al.conformers[r]) and f[3] == "nodes"
        assert int(f[4]) == int(clash_rows[r][6]) and f[5] == clash_rows[r][8] and float(f[5]) == ref.overlap_start[r]
        assert int(f[6]) == ref.n_pairs[r] == rep.n_pairs[r] and float(f[7]) == ref.overlap[r] and repr(float(f[7])) == f[7]
        assert float(f[8]) == rep.clearance[r] and int(f[9]) == rep.n_clashing[r] and float(f[10]) == ref.anchor_rmsd[r]
        assert float(f[11]) == float(np.degrees(ref.angle[r])) and float(f[12]) == ref.shift[r] and (int(f[13]), int(f[14])) == (ref.iterations[r], ref.stop[r])
        assert np.array_equal(np.array([float(v) for v in f[15:24]]).reshape(3, 3), ref.rotation[r]) and np.array_equal(np.array([float(v) for v in f[24:27]]), ref.translation[r])
