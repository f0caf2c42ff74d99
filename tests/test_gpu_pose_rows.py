"""The posed-row calls - `clashes`, `shape`, `overlay`, `overlay_starts`, `refine`, `pose_fit` - share one Python call frame
(`poses._pose_frame`) and one row front end on the device (`pose_motion` and `pose_row` of csrc/pmx_pose.h): the same rows, good and bad,
mean the same thing to every one of them, in each of the three sources of points."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_pose_calls_agree_on_what_a_row_is():
    """One OK hit of set_6oim_c8 under its own fitted pose, and what can be wrong with a row: a conformer the record lacks (C and -1), a
    ligand outside the library, a motion that is not finite. Node mode through all six calls, point mode with the record's own node
    positions (the same float32 coordinates and the same radius: the same bits), the atom store with a ligand it has no atoms for, and
    calls without a row. `overlay_starts` reads no motion, so the NaN costs its row nothing. The store's expected statuses, NaN and
    `indices` are what the calls returned before they shared the frame."""
    from pharmaconet_amd.atoms import PackedAtoms
    from pharmaconet_amd.engine import clashes, overlay, overlay_starts, pose_fit, refine, shape
    from test_gpu_align import posed
    from test_gpu_atoms import store_6oim
    from test_gpu_clash import pocket_6oim
    from test_gpu_pose_shape import golden_reference

    model, lib, weights, ex, al = posed("set_6oim_c8")
    pocket, reference = pocket_6oim(), golden_reference()
    r0 = int(np.flatnonzero(al.status == 0)[0])
    lig, c, R, t = int(al.indices[r0]), int(al.conformers[r0]), al.rotation[r0], al.translation[r0]
    nn, C, _ = lib.header(lig)
    assert C == 8 and 0 <= c < C and nn >= 2
    Rnan = R.copy()
    Rnan[1, 2] = np.nan
    idx, conf = [lig, lig, lig, len(lib), lig], [c, C, -1, 0, c]
    rot, trans = np.stack([R, R, R, R, Rnan]), np.stack([t] * 5)

    # ---- node mode
    node = dict(library=lib, indices=idx, conformers=conf)
    cl = clashes(pocket, rotation=rot, translation=trans, **node)
    sh = shape(reference, rotation=rot, translation=trans, **node)
    ov = overlay(reference, rotation=rot, translation=trans, max_iter=0, **node)
    rf = refine(pocket, rotation=rot, translation=trans, max_iter=0, **node)
    pf = pose_fit(model, lib, idx, conf, rot, trans, weights=weights)
    for name, out in (("clashes", cl), ("shape", sh), ("overlay", ov), ("refine", rf), ("pose_fit", pf)):
        assert out.status.tolist() == [0, 4, 4, 1, 4], name
        assert len(out) == 5, name
    for name, lists in (("clashes", cl.point_penetration), ("clashes", cl.point_atom), ("shape", sh.point_distance), ("shape", sh.point_reference_atom),
                        ("pose_fit", pf.node_fit), ("pose_fit", pf.node_target)):
        assert [len(v) for v in lists] == [nn, nn, nn, 0, nn], name
    for out in (ov, rf):  # a row that is not OK has no motion; the OK row keeps its own at max_iter=0
        assert np.array_equal(out.rotation[0], R) and np.array_equal(out.translation[0], t)
        assert np.isnan(out.rotation[1:]).all() and np.isnan(out.translation[1:]).all() and out.stop.tolist() == [out.stop[0], -1, -1, -1, -1]
        assert out.indices.tolist() == idx and out.conformers.tolist() == conf
    starts = overlay_starts(reference, [0] * 5, **node)
    assert starts.status.tolist() == [0, 4, 4, 1, 0]
    assert np.array_equal(starts.rotation[0], starts.rotation[4]) and np.isfinite(starts.rotation[0]).all() and np.isfinite(starts.axes[4]).all()
    assert np.isnan(starts.rotation[1:4]).all() and np.isnan(starts.translation[1:4]).all() and np.isnan(starts.centre[1:4]).all() and np.isnan(starts.values[1:4]).all()

    # ---- point mode: the record's own node positions at conformer c
    pts = np.ascontiguousarray(lib.unpack(lig)["xyz"][:, :, c])
    assert pts.dtype == np.float32 and pts.shape == (nn, 3)
    two = dict(points=[pts, pts], rotation=rot[[0, 4]], translation=trans[[0, 4]])
    pcl, psh = clashes(pocket, **two), shape(reference, **two)
    pov, prf = overlay(reference, max_iter=0, **two), refine(pocket, max_iter=0, **two)
    for name, out in (("clashes", pcl), ("shape", psh), ("overlay", pov), ("refine", prf)):
        assert out.status.tolist() == [0, 4], name
    assert pov.indices is None and prf.indices is None and overlay_starts(reference, [0, 0], points=[pts, pts]).status.tolist() == [0, 0]
    same = lambda a, b: np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)  # noqa: E731
    for f in ("clearance", "overlap", "n_points", "n_clashing", "n_pairs", "n_contacts", "worst", "contact_fingerprint"):
        assert same(getattr(pcl, f)[0], getattr(cl, f)[0]), f
    assert same(pcl.point_penetration[0], cl.point_penetration[0]) and same(pcl.point_atom[0], cl.point_atom[0])
    for f in ("overlap", "self_overlap", "reference_overlap", "tanimoto", "reference_fraction", "fit_fraction", "rms_to_reference", "rms_from_reference", "rmsd_in_order",
              "n_points", "n_covered", "n_reference_covered"):
        assert same(getattr(psh, f)[0], getattr(sh, f)[0]), f
    for f in ("overlap_start", "overlap", "tanimoto", "n_points"):
        assert same(getattr(pov, f)[0], getattr(ov, f)[0]), f
    assert same(prf.overlap[0], rf.overlap[0]) and same(prf.rotation[0], rf.rotation[0])

    # ---- the atom store: the hit, a conformer it lacks, and a ligand the store has no atoms for (as for an unsupported record)
    _, mols = store_6oim()
    other = next(i for i in range(len(lib)) if i != lig)
    keep = np.ones(len(lib), bool)
    keep[other] = False
    store = dict(atoms=PackedAtoms.from_features(mols, keep), indices=[lig, lig, other], conformers=[c, C, 0])
    three = dict(rotation=rot[:3], translation=trans[:3])
    scl, ssh = clashes(pocket, **three, **store), shape(reference, **three, **store)
    sov, srf = overlay(reference, max_iter=0, **three, **store), refine(pocket, max_iter=0, **three, **store)
    sst = overlay_starts(reference, [0, 0, 0], **store)
    got = {name: out.status.tolist() for name, out in (("clashes", scl), ("shape", ssh), ("overlay", sov), ("refine", srf), ("overlay_starts", sst))}
    print(f"store-mode statuses: {got}")
    assert got == {name: [0, 4, 1] for name in got}
    assert scl.n_points[0] == ssh.n_points[0] == sov.n_points[0] > 0 and scl.n_points.tolist()[1:] == [0, 0] and [len(v) for v in ssh.point_distance[1:]] == [0, 0]
    for out in (sov, srf, sst):
        assert np.isfinite(out.rotation[0]).all() and np.isnan(out.rotation[1:]).all() and np.isnan(out.translation[1:]).all()
    assert np.isnan(sst.centre[1:]).all() and np.isnan(sst.axes[1:]).all() and np.isnan(sst.values[1:]).all() and np.isfinite(sst.axes[0]).all()
    assert sov.indices.tolist() == [lig, lig, other] and sov.conformers.tolist() == [c, C, 0]
    assert srf.indices is None and srf.conformers is None  # (`refine` names its rows in node mode only)
    four = overlay(reference, starts=4, **store)  # (the inertial leg: one hit per row, four starts each)
    assert four.status.tolist() == [0, 4, 1] and four.start.tolist()[1:] == [0, 0] and np.isnan(four.rotation[1:]).all() and np.isnan(four.start_tanimoto[1:]).all()

    # ---- no rows
    none = dict(library=lib, indices=[], conformers=[])
    no_motion = dict(rotation=np.zeros((0, 3, 3)), translation=np.zeros((0, 3)))
    for name, out in (("clashes", clashes(pocket, **none, **no_motion)), ("shape", shape(reference, **none, **no_motion)), ("overlay", overlay(reference, **none, **no_motion)),
                      ("refine", refine(pocket, **none, **no_motion)), ("pose_fit", pose_fit(model, lib, [], [], **no_motion)),
                      ("overlay_starts", overlay_starts(reference, [], **none)), ("overlay starts=4", overlay(reference, starts=4, **none))):
        assert len(out) == 0 and out.status.shape == (0,) and out.status.dtype == np.int32, name
