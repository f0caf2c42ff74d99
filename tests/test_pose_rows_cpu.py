"""The host side of the posed-row calls without a GPU: what `_PoseRows` refuses and how it lays rows out, what the posed result classes
(`Alignment`, `RefinedPoses`, `ShapeOverlay`) share through `poses._PosedRows`, and that `engine` still hands out every name the rest of
the repository takes from it. NumPy only: nothing here reaches the device."""

import dataclasses

import numpy as np
import pytest

from pharmaconet_amd.engine import _PoseRows

EYE2, ZERO2 = np.broadcast_to(np.eye(3), (2, 3, 3)), np.zeros((2, 3))
LIB = object()  # (`_PoseRows` asks only whether there is a library)


def rows(library=None, indices=None, conformers=None, rotation=EYE2, translation=ZERO2, points=None, point_radii=None, atoms=None):
    return _PoseRows("clashes", library, indices, conformers, rotation, translation, points, point_radii, atoms)


# ---------------------------------------------------------------------------------------------------------------- 1. _PoseRows
PTS = [np.zeros((3, 3)), np.zeros((1, 3))]
REFUSED = [
    (dict(library=LIB, indices=[0, 1], conformers=[0, 0], translation=np.zeros((3, 3))), ValueError, "rotation and translation differ in length"),
    (dict(library=LIB, indices=[0, 1], conformers=[0, 0], points=PTS), ValueError, "clashes: a library with indices and conformers, or points - one of the two"),
    (dict(atoms="a store", indices=[0, 1], conformers=[0, 0]), TypeError, "clashes: atoms is a DeviceAtoms or a PackedAtoms"),
    (dict(), ValueError, "clashes: a library with indices and conformers, or points - one of the two"),
    (dict(library=LIB, indices=np.zeros(65537, np.int64), conformers=np.zeros(65537, np.int64), rotation=np.zeros((65537, 3, 3)), translation=np.zeros((65537, 3))),
     ValueError, "at most 65536 rows per clashes call (PMX_EXPLAIN_MAX)"),
    (dict(library=LIB, indices=[0, -1], conformers=[0, 0]), ValueError, "negative ligand index"),
    (dict(library=LIB, indices=[0], conformers=[0, 0]), ValueError, "indices, conformers and the motions differ in length"),
    (dict(library=LIB, indices=[0, 1], conformers=[0]), ValueError, "indices, conformers and the motions differ in length"),
    (dict(points=PTS[:1]), ValueError, "1 point sets for 2 motions"),
    (dict(points=PTS, point_radii=[np.ones(3)]), ValueError, "1 radius lists for 2 point sets"),
    (dict(points=PTS, point_radii=[np.ones(2), np.ones(1)]), ValueError, "a list of radii differs in length from its points"),
]


@pytest.mark.parametrize("kw, error, message", REFUSED, ids=[r[2][:40] + f" [{i}]" for i, r in enumerate(REFUSED)])
def test_pose_rows_refuses(kw, error, message):
    with pytest.raises(error) as e:
        rows(**kw)
    assert str(e.value) == message and type(e.value) is error


def test_pose_rows_refuses_an_atom_store_next_to_another_source():
    from pharmaconet_amd.atoms import PackedAtoms

    store = PackedAtoms.from_arrays([[6, 8]], [np.zeros((2, 1, 3), np.float32)])
    message = "clashes: a library, points or an atom store - exactly one source of points"
    for kw in (dict(points=PTS), dict(library=LIB), dict(point_radii=[np.ones(3), np.ones(1)])):
        with pytest.raises(ValueError) as e:
            rows(atoms=store, indices=[0, 0], conformers=[0, 0], **kw)
        assert str(e.value) == message
    r = rows(atoms=store, indices=[0, 0], conformers=[0, 7])
    assert not r.node_mode and r.store is store and r.idx.tolist() == [0, 0] and r.conf.tolist() == [0, 7] and r.off is None and r.gstatus is None


def check_motions(r, n):
    assert r.n == n and r.rot.dtype == r.trans.dtype == np.float64 and r.rot.shape == (n, 3, 3) and r.trans.shape == (n, 3)
    assert r.rot.flags.c_contiguous and r.trans.flags.c_contiguous and r.gstatus is None and r.store is None


def test_pose_rows_lays_node_rows_out():
    for n in (0, 1, 2):
        R, t = np.arange(9.0 * n).reshape(n, 3, 3), np.arange(3.0 * n).reshape(n, 3)
        r = rows(library=LIB, indices=list(range(5, 5 + n)), conformers=[2**40, -7][:n], rotation=R, translation=t)
        check_motions(r, n)
        assert r.node_mode and np.array_equal(r.rot, R) and np.array_equal(r.trans, t)
        assert r.idx.dtype == np.int64 and r.idx.tolist() == list(range(5, 5 + n))
        assert r.conf.dtype == np.int32 and r.conf.tolist() == [2**31 - 1, -1][:n]  # (clipped to what the C ABI's int32 holds)
        assert r.off is None and r.flat is None and r.rad is None


def test_pose_rows_lays_point_rows_out():
    a = np.arange(9, dtype=np.float64).reshape(3, 3)
    for pts, radii, off in (([], [], [0]), ([a], [[1, 2, 3]], [0, 3]), ([a, np.zeros((0, 3))], [[1, 2, 3], []], [0, 3, 3]), ([np.zeros((0, 3)), a], None, [0, 0, 3])):
        n = len(pts)
        r = rows(points=pts, point_radii=radii, rotation=EYE2[:n], translation=ZERO2[:n])
        check_motions(r, n)
        total = off[-1]
        assert not r.node_mode and r.idx is None and r.conf is None
        assert r.off.dtype == np.int64 and r.off.tolist() == off
        assert r.flat.dtype == np.float32 and r.flat.shape == (total + 1, 3) and r.flat.flags.c_contiguous  # (one row of padding: never an empty buffer)
        assert np.array_equal(r.flat[:total], a.astype(np.float32)[:total]) and not r.flat[total].any()
        if radii is None:
            assert r.rad is None
        else:
            assert r.rad.dtype == np.float32 and r.rad.shape == (total + 1,) and r.rad[:total].tolist() == [1.0, 2.0, 3.0][:total]
        assert r.finish(np.array([0, 4][:n], np.int32)).tolist() == [0, 4][:n]  # (no gather: the call's own statuses)


# ---------------------------------------------------------------------------------------------------------------- 2. the posed result classes
PUBLIC = {
    "Alignment": {"clashes", "overlay", "pose_fit", "refine", "shape", "transform"},
    "RefinedPoses": {"clashes", "overlay", "pose_fit", "shape", "transform"},
    "ShapeOverlay": {"clashes", "pose_fit", "refine", "shape", "transform"},
}


def by_hand(name, **given):
    """Two rows of class `name`, every field that is not given a pair of zeros."""
    from pharmaconet_amd import engine

    cls = getattr(engine, name)
    rng = np.random.default_rng(5)
    Q = np.linalg.qr(rng.normal(size=(2, 3, 3)))[0]
    values = dict(rotation=Q, translation=rng.normal(size=(2, 3)), indices=np.array([3, 4]), conformers=np.array([0, 1]))
    values.update(given)
    return cls(**{f.name: values.get(f.name, np.zeros(2)) for f in dataclasses.fields(cls)})


@pytest.mark.parametrize("name", sorted(PUBLIC))
def test_posed_classes_share_their_methods(name):
    from pharmaconet_amd import engine

    poses = by_hand(name)
    assert len(poses) == 2
    x = np.random.default_rng(6).normal(size=(4, 5, 3))
    for i in range(2):
        assert np.array_equal(poses.transform(i, x), x @ poses.rotation[i].T + poses.translation[i])
    cls = getattr(engine, name)
    assert {k for k in dir(cls) if not k.startswith("_") and callable(getattr(cls, k))} == PUBLIC[name]
    with pytest.raises(ValueError) as e:
        poses.clashes(None, library=None, atoms=None)
    assert str(e.value) == f"{name}.clashes: the library the rows are ligands of, or `atoms`"
    with pytest.raises(ValueError) as e:
        poses.shape(None)
    assert str(e.value) == f"{name}.shape: the library the rows are ligands of, or `atoms`"


def test_rows_that_are_points_of_the_callers_have_no_library_methods():
    ov = by_hand("ShapeOverlay", indices=None, conformers=None)
    with pytest.raises(ValueError) as e:
        ov.refine(None)
    assert str(e.value) == "ShapeOverlay.refine: these rows are points of the caller's, not ligands of a library"
    with pytest.raises(ValueError) as e:
        ov.pose_fit(None, None)
    assert str(e.value) == "ShapeOverlay.pose_fit: these rows are points of the caller's, not ligands of a library"
    with pytest.raises(ValueError) as e:
        by_hand("RefinedPoses", indices=None, conformers=None).pose_fit(None, None)
    assert str(e.value) == "RefinedPoses.pose_fit: these rows are points of the caller's, not ligands of a library"
    with pytest.raises(ValueError) as e:
        by_hand("Alignment").overlay(None, starts=4)
    assert str(e.value) == "Alignment.overlay: the local overlay of these poses; `overlay(..., starts=4)` is the one that needs no pose"


# ---------------------------------------------------------------------------------------------------------------- 3. engine stays the public module
# every name a file of the repository takes from `pharmaconet_amd.engine` (bench.py, __graft_entry__.py, tests/, tools/ and the package's own modules)
TAKEN_FROM_ENGINE = (
    "Attribution", "DeviceAtoms", "DeviceLibrary", "DiverseHits", "ENRICH_TILE", "FEATURE_FIELDS", "ModeSet", "POISSON1_CDF64", "ScreeningResult", "_ModelHandle",
    "_atomic_numbers", "_constraint_struct", "_device_index", "_explain_call", "_explain_rows", "_heavy_atoms", "_listed_rows", "_pose_source", "_resident_atoms",
    "_search_chunks", "_weights_array", "align", "attribute", "clashes", "cutoffs_ppm", "device_model", "device_pocket", "device_shape_ref", "enrichment", "explain",
    "explain_modes", "features_to_device", "fingerprint_leaders", "fingerprint_similarity", "hotspots", "key_qualifies", "last_score_stats", "normalize_constraint", "overlay",
    "overlay_starts", "pack_bound", "pack_features_device", "pose_fit", "pose_search", "refine", "release_workspaces", "score_one", "screen", "screen_constrained",
    "screen_multi", "set_profiling", "shape", "similar", "sweep", "topk",
    # ... and the classes and helpers of the layers below that a caller may hold by their old path
    "Alignment", "ClashReport", "PoseFit", "RefinedPoses", "ShapeOverlay", "ShapeReport", "ShapeStarts", "PoseSearch", "FittingHits", "_PoseRows", "_resident", "_listed_indices",
    "_torch", "_record_counts", "NO_MATCH", "NO_LEVEL", "KEY_INVALID",
)


def test_engine_hands_out_every_name_it_did():
    from pharmaconet_amd import _device, engine, poses

    missing = [n for n in TAKEN_FROM_ENGINE if not hasattr(engine, n)]
    assert not missing, missing
    for layer in (poses, _device):  # a name of a lower layer is the same object up here
        for n in TAKEN_FROM_ENGINE:
            if hasattr(layer, n):
                assert getattr(engine, n) is getattr(layer, n), n
    assert engine.clashes is poses.clashes and engine.pose_fit is poses.pose_fit and engine.Alignment is poses.Alignment
    assert engine.DeviceLibrary is _device.DeviceLibrary and engine._ModelHandle is _device._ModelHandle and engine._device_index is _device._device_index
    for cls in (engine.Alignment, engine.RefinedPoses, engine.ShapeOverlay):
        assert issubclass(cls, poses._PosedRows)
    for cls in (_device._ModelHandle, poses._PocketHandle, poses._ShapeRefHandle):
        assert issubclass(cls, _device._DeviceHandle) and cls._destroy and "__del__" not in vars(cls)
