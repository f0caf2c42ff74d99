"""`pmx_pose_colour` on the GPU (csrc/pmx_colour.hip) against the NumPy restatement of tests/colour_ref.py over the seeded rows of
tests/combo_cases.py: feature mode over every case, node mode on the same rows as records of a library and on a golden set, the
consequences that must hold exactly, repeatability, statuses, the host's refusals, and the Python layer on top of it.

Bars. Integers and indices (status, counts, nearest partners, the matched fingerprint) must be equal; they can differ only where a row
stands within rounding of a decision, so they are asserted after the restatement's `margin` is at least 1e-9 on every row (checked on the
CPU by tests/test_colour_cpu.py). Distances are within 1e-12 * max(1, |v|): square roots of sums of three correctly rounded products.
Overlaps are within 1e-13 * v + 1e-300, the bar and the argument of tests/test_gpu_pose_shape.py: sums of terms that are >= 0 - the
weights are - and differ from the restatement's through `exp` alone, so the relative error of a sum is at most that of its worst term.
Ratios are exactly the header's formulas applied to the device's own three overlaps."""

import ctypes
from functools import lru_cache

import numpy as np
import pytest

import colour_ref
import combo_cases
import shape_ref
from combo_cases import COLOUR_RADIUS, COVER, MARGIN
from conftest import load_golden

pytestmark = pytest.mark.gpu

EYE, ZERO = np.eye(3), np.zeros(3)
FIELDS = ("overlap", "self_overlap", "reference_overlap", "tanimoto", "reference_fraction", "fit_fraction", "rms_matched", "type_overlap", "n_nodes", "n_matched",
          "n_reference_features", "n_reference_matched", "matched_fingerprint", "status")
LISTS = ("node_overlap", "node_distance", "node_feature", "feature_distance", "feature_node")


def weights_dict(w):
    from pharmaconet_amd.constants import TYPE_NAMES

    return {name: float(w[t]) for t, name in enumerate(TYPE_NAMES)}


@lru_cache(maxsize=None)
def case_ref(name):
    from pharmaconet_amd.shape import ColourFeatures

    c = combo_cases.case(name)
    return ColourFeatures.from_arrays(c["feat_xyz"], c["feat_mask"], weights=weights_dict(c["weights"]), radius=COLOUR_RADIUS)


def run(name, rows=None, node_mode=False, **kw):
    from pharmaconet_amd.engine import colour

    c = combo_cases.case(name)
    rows = list(range(c["n"])) if rows is None else [int(i) for i in rows]
    args = dict(cover=COVER)
    args.update(kw)
    if node_mode:
        lib, conf = combo_cases.library(name)
        return colour(case_ref(name), lib, rows, conf[rows], c["R"][rows], c["t"][rows], **args)
    return colour(case_ref(name), rotation=c["R"][rows], translation=c["t"][rows], features=[c["nodes"][i] for i in rows], feature_types=[c["masks"][i] for i in rows], **args)


@lru_cache(maxsize=None)
def result(name):
    return run(name)


def same_bits(a, b, rows=None):
    rows = np.arange(len(b)) if rows is None else np.asarray(rows)
    if len(a) != len(rows) or not all(np.array_equal(getattr(a, f), getattr(b, f)[rows], equal_nan=True) for f in FIELDS):
        return False
    return all(np.array_equal(getattr(a, f)[k], getattr(b, f)[int(i)], equal_nan=True) for f in LISTS for k, i in enumerate(rows))


def close(got, want, rel, floor):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    both_nan = np.isnan(got) & np.isnan(want)
    return bool((both_nan | (np.abs(got - want) <= rel * np.abs(want) + floor)).all())


def near(got, want):
    """Distances: within 1e-12 * max(1, |v|), NaN where the restatement has NaN."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool(((np.isnan(got) & np.isnan(want)) | (np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want)))).all())


def header_ratios(out, i):
    cab, caa, cbb = np.float64(out.overlap[i]), np.float64(out.self_overlap[i]), np.float64(out.reference_overlap[i])
    with np.errstate(all="ignore"):
        return [0.0 if cab == 0 else cab / ((caa + cbb) - cab), 0.0 if cbb == 0 else cab / cbb, 0.0 if caa == 0 else cab / caa]


def check_against(out, refs, tag):
    """Every row of `out` against the restatement's rows; the worst figures are printed before anything is asserted."""
    assert len(out) == len(refs), tag
    margin = min([r["margin"] for r in refs], default=np.inf)
    worst_o = worst_d = 0.0
    for i, r in enumerate(refs):
        if r["status"] != 0 or out.status[i] != 0:
            continue
        n, f = int(r["counts"][0]), int(r["counts"][3])
        for got, want in ((out.overlap[i], r["summary"][0]), (out.self_overlap[i], r["summary"][1]), *zip(out.type_overlap[i], r["type_overlap"]), *zip(out.node_overlap[i], r["node_colour"][:n])):
            if want > 0:
                worst_o = max(worst_o, abs(got - want) / want)
        for got, want in (*zip(out.node_distance[i], r["node_near"][:n]), *zip(out.feature_distance[i], r["feat_near"][:f]), (out.rms_matched[i], r["summary"][6])):
            if np.isfinite(want):
                worst_d = max(worst_d, abs(got - want) / max(1.0, abs(want)))
    print(f"{tag}: rows {len(refs)} margin {margin:.3e} worst relative overlap error {worst_o:.3e} (bar 1e-13), worst distance error {worst_d:.3e} (bar 1e-12)")
    assert margin >= MARGIN, (tag, margin)
    for i, r in enumerate(refs):
        assert out.status[i] == r["status"], (tag, i)
        n, f = (int(r["counts"][0]), int(r["counts"][3])) if r["status"] == 0 else (0, len(out.feature_node[i]))
        got = [int(out.n_nodes[i]), int(out.n_matched[i]), int(out.n_reference_matched[i]), int(out.n_reference_features[i])]
        assert got == r["counts"].tolist(), (tag, i, got, r["counts"])
        assert np.array_equal(out.node_feature[i], r["node_feature"][:n]) and np.array_equal(out.feature_node[i], r["feat_node"][:f]), (tag, i)
        assert out.matched_fingerprint[i].tolist() == [r["fp"], 0, 0, 0], (tag, i)
        if r["status"] != 0:
            assert np.isnan(out.overlap[i]) and np.isnan(out.tanimoto[i]) and np.isnan(out.type_overlap[i]).all() and np.isnan(out.feature_distance[i]).all(), (tag, i)
            continue
        assert near(out.node_distance[i], r["node_near"][:n]) and near(out.feature_distance[i], r["feat_near"][:f]) and near(out.rms_matched[i], r["summary"][6]), (tag, i)
        assert close(out.overlap[i], r["summary"][0], 1e-13, 1e-300) and close(out.self_overlap[i], r["summary"][1], 1e-13, 1e-300), (tag, i)
        assert close(out.type_overlap[i], r["type_overlap"], 1e-13, 1e-300) and close(out.node_overlap[i], r["node_colour"][:n], 1e-13, 1e-300), (tag, i)
        assert [out.tanimoto[i], out.reference_fraction[i], out.fit_fraction[i]] == header_ratios(out, i), (tag, i)
        assert (out.type_overlap[i] >= 0).all() and abs(out.type_overlap[i].sum() - out.overlap[i]) <= 1e-12 * out.overlap[i], (tag, i)


# ---------------------------------------------------------------------------------------------------------------- 1. against the restatement
@pytest.mark.parametrize("name", list(combo_cases.CASES))
def test_feature_mode_against_the_restatement(name):
    c = combo_cases.case(name)
    out = result(name)
    check_against(out, combo_cases.colour_reference(name), name)
    assert (out.status == 0).all() and (out.reference_overlap == case_ref(name)._device[out.device].self_overlap).all()
    assert close(out.reference_overlap[0], c["c_bb"], 1e-13, 0.0)
    assert {0, 1, 2, 63, 64} <= set(out.n_nodes.tolist())


@pytest.mark.parametrize("name", ["f63", "f2_nodes"])
def test_node_mode_reads_the_records_and_has_feature_modes_bits(name):
    out = run(name, node_mode=True)
    assert same_bits(out, result(name))


def test_node_mode_on_a_golden_set():
    """The known binder is ligand 5 of the set at its conformer 0 under a motion; the rows are the set's ligands at their first and last
    conformers under random motions near it."""
    from pharmaconet_amd.engine import colour
    from pharmaconet_amd.shape import ColourFeatures

    _, lib, _, _ = load_golden("set_6oim_c8")
    rng = np.random.default_rng(8)
    heads = lib.headers()
    idx = np.concatenate([np.arange(min(len(lib), 24))] * 2)
    conf = np.concatenate([np.zeros(len(idx) // 2, np.int64), heads[idx[: len(idx) // 2], 1].astype(np.int64) - 1])
    R, t = shape_ref.random_rotations(rng, len(idx)), rng.uniform(-1.5, 1.5, size=(len(idx), 3))
    R[5], t[5] = EYE, ZERO
    ref = ColourFeatures.from_library(lib, 5, 0, radius=COLOUR_RADIUS)
    out = colour(ref, lib, idx, conf, R, t, cover=COVER)
    w = ref.weights_array()
    c_bb = colour_ref.self_overlap(ref.xyz, ref.typemask, w, COLOUR_RADIUS)
    refs = []
    for i in range(len(idx)):
        rec = lib.unpack(int(idx[i]))
        refs.append(colour_ref.colour_row(ref.xyz, ref.typemask, w, COLOUR_RADIUS, rec["xyz"][:, :, int(conf[i])], rec["typemask"], R[i], t[i], COVER, c_bb=c_bb))
    check_against(out, refs, "node mode, set_6oim_c8")
    assert (out.status == 0).all() and np.array_equal(out.n_nodes, heads[idx, 0])
    # row 5 is the binder itself in place
    assert out.overlap[5] == out.self_overlap[5] == out.reference_overlap[5] and out.tanimoto[5] == 1.0 and out.n_matched[5] == out.n_reference_matched[5]
    assert set(out.by_type(5)) == {"Hydrophobic", "Aromatic", "Cation", "Anion", "HBond_donor", "HBond_acceptor", "Halogen"} and sum(out.by_type(5).values()) > 0


# ---------------------------------------------------------------------------------------------------------------- 2. what is exact
def test_exact_consequences():
    from pharmaconet_amd.engine import colour
    from pharmaconet_amd.shape import ColourFeatures

    for name in ("f1", "f2_nodes", "f63", "f64"):
        c = combo_cases.case(name)
        ref = case_ref(name)
        own = colour(ref, rotation=[EYE], translation=[ZERO], features=[c["feat_xyz"]], feature_types=[c["feat_mask"]])
        assert own.overlap[0] == own.self_overlap[0] == own.reference_overlap[0] > 0 and own.tanimoto[0] == 1.0 and own.reference_fraction[0] == 1.0, name
        assert own.rms_matched[0] == 0.0 and own.n_matched[0] == own.n_reference_matched[0], name
    one = ColourFeatures.from_arrays([[1.0, 2.0, 3.0]], np.array([0b1100], np.uint8), radius=1.0)
    q = shape_ref.PI / (colour_ref.alpha_c(1.0) + colour_ref.alpha_c(1.0))
    pts, far = np.array([[1.0, 2.0, 3.0]], np.float32), np.array([[201.0, 2.0, 3.0]], np.float32)
    out = colour(one, rotation=[EYE] * 4, translation=[ZERO] * 4, features=[pts, far, pts, pts],
                 feature_types=[np.array([0b0101], np.uint8), np.array([0b0101], np.uint8), np.array([0b0011], np.uint8), np.array([0b1100], np.uint8)])
    assert out.overlap[0] == 8.0 * (8.0 * (q * np.sqrt(q))) and out.by_type(0)["Cation"] == out.overlap[0] and out.by_type(0)["Anion"] == 0.0  # one shared type, weight 8
    assert out.overlap[1] == 0.0 and out.tanimoto[1] == 0.0 and out.node_feature[1][0] == 0 and out.n_matched[1] == 0 and out.matched_fingerprint[1].tolist() == [0, 0, 0, 0]
    assert out.overlap[2] == 0.0 and out.tanimoto[2] == 0.0 and out.node_feature[2][0] == -1 and np.isnan(out.rms_matched[2]) and out.self_overlap[2] > 0  # no shared type
    assert out.overlap[3] == (8.0 + 8.0) * (8.0 * (q * np.sqrt(q))) and out.tanimoto[3] == 1.0 and out.matched_fingerprint[3].tolist() == [1, 0, 0, 0]
    # every type the row has is zero-weighted
    zero = ColourFeatures.from_arrays([[1.0, 2.0, 3.0]], ["Hydrophobic"], weights={"Hydrophobic": 0.0})
    out = colour(zero, rotation=[EYE], translation=[ZERO], features=[pts], feature_types=[["Hydrophobic"]])
    assert out.overlap[0] == 0.0 and out.tanimoto[0] == 0.0 and out.self_overlap[0] == 0.0 and out.reference_overlap[0] == 0.0 and out.fit_fraction[0] == 0.0
    assert out.reference_fraction[0] == 0.0 and out.node_feature[0][0] == -1 and out.status[0] == 0


@pytest.mark.parametrize("n", [1, 4, 5, 64])
def test_row_counts_and_the_same_bits_wherever_a_row_stands(n):
    name = "f63"
    whole = result(name)
    pick = ([4, 2, 12, 5, 0] + list(range(13, 72)))[:n]
    pick = [i % 64 for i in pick]
    out = run(name, rows=pick)
    assert same_bits(out, whole, rows=pick)
    assert same_bits(run(name, rows=pick), out)  # two runs
    if n == 64:
        perm = np.random.default_rng(3).permutation(64)
        assert same_bits(run(name, rows=perm), whole, rows=perm)


# ---------------------------------------------------------------------------------------------------------------- 3. rows that are not OK
def test_every_status_that_is_not_ok():
    from pharmaconet_amd.engine import colour

    name = "f63"
    c = combo_cases.case(name)
    ref = case_ref(name)
    lib, conf = combo_cases.library(name)
    bad_R = EYE.copy()
    bad_R[0, 1] = np.nan
    idx = [3, 3, 3, 64, 3]
    out = colour(ref, lib, idx, [1, 2, -1, 0, 1], [EYE, EYE, EYE, EYE, bad_R], [ZERO, ZERO, ZERO, ZERO, ZERO])
    assert out.status.tolist() == [0, 4, 4, 1, 4]
    many = np.zeros((65, 3), np.float32)
    feat = colour(ref, rotation=[EYE, EYE, EYE, EYE], translation=[ZERO, ZERO, np.array([np.inf, 0, 0]), ZERO], features=[c["nodes"][3], many, c["nodes"][3], c["nodes"][4]],
                  feature_types=[c["masks"][3], np.ones(65, np.uint8), c["masks"][3], np.where(np.arange(len(c["masks"][4])) == 40, 128, c["masks"][4]).astype(np.uint8)])
    assert feat.status.tolist() == [0, 1, 4, 4]
    for rep, bad in ((out, [1, 2, 3, 4]), (feat, [1, 2, 3])):
        for i in bad:
            assert all(np.isnan(getattr(rep, f)[i]).all() for f in FIELDS[:8]) and all(getattr(rep, f)[i] == 0 for f in FIELDS[8:12]), i
            assert rep.matched_fingerprint[i].tolist() == [0, 0, 0, 0] and len(rep.node_feature[i]) == 0 and (rep.feature_node[i] == -1).all() and np.isnan(rep.feature_distance[i]).all()
    assert same_bits(colour(ref, lib, [3], [1], [EYE], [ZERO]), out, rows=[0])


def raw_create(xyz, mask, weights, radius, device=0):
    from pharmaconet_amd import _ffi

    xyz, mask = np.ascontiguousarray(xyz, dtype=np.float32), np.ascontiguousarray(mask, dtype=np.uint8)
    handle = ctypes.c_void_p()
    rc = _ffi.load().pmx_colour_ref_create(xyz.ctypes.data, mask.ctypes.data, len(mask), (ctypes.c_float * 7)(*weights), radius, device, ctypes.byref(handle))
    return rc, handle


def test_the_hosts_refusals_and_no_rows():
    import torch

    from pharmaconet_amd import _ffi
    from pharmaconet_amd.engine import colour, device_colour_ref

    lib = _ffi.load()
    w = list(combo_cases.DEFAULT)
    ok_xyz, ok_mask = np.zeros((2, 3), np.float32), [1, 2]
    rc, handle = raw_create(ok_xyz, ok_mask, w, 1.0)
    assert rc == 0 and handle.value
    out = ctypes.c_double()
    assert lib.pmx_colour_ref_self(handle, ctypes.byref(out)) == 0 and out.value > 0 and lib.pmx_colour_ref_self(None, ctypes.byref(out)) != 0
    nan_xyz = ok_xyz.copy()
    nan_xyz[1, 2] = np.inf
    for args in ((np.zeros((0, 3)), [], w, 1.0), (np.zeros((65, 3)), [1] * 65, w, 1.0), (ok_xyz, [1, 128], w, 1.0), (ok_xyz, ok_mask, [-1.0] + w[1:], 1.0),
                 (ok_xyz, ok_mask, w[:6] + [float("nan")], 1.0), (ok_xyz, ok_mask, w, 0.0), (ok_xyz, ok_mask, w, -1.0), (ok_xyz, ok_mask, w, float("inf")), (nan_xyz, ok_mask, w, 1.0)):
        rc, bad = raw_create(*args)
        assert rc != 0 and not bad.value and b"pmx_colour_ref_create" in lib.pmx_last_error(), args[1:]
    assert lib.pmx_colour_ref_create(None, None, 2, (ctypes.c_float * 7)(*w), 1.0, 0, None) != 0
    # the call itself
    dev = torch.device("cuda", 0)
    z = lambda *s, dt=torch.float64: torch.zeros(s, dtype=dt, device=dev)  # noqa: E731
    rot, trans, off, pts, mk = z(1, 9), z(1, 3), z(2, dt=torch.int64), z(1, 3, dt=torch.float32), z(1, dt=torch.uint8)
    outs = [z(1, 8), z(1, 7), z(1, 4, dt=torch.int32), z(1, 64), z(1, 64), z(1, 64, dt=torch.int32), z(1, 64), z(1, 64, dt=torch.int32), z(1, 4, dt=torch.int64), z(1, dt=torch.int32)]
    ptrs = [o.data_ptr() for o in outs]
    call = lambda ref, n, cover=2.0, source=(None, None, None, off.data_ptr(), pts.data_ptr(), mk.data_ptr()), o=ptrs: lib.pmx_pose_colour(  # noqa: E731
        ref, *source, rot.data_ptr(), trans.data_ptr(), n, cover, *o, None)
    assert call(None, 1) != 0 and b"null reference" in lib.pmx_last_error()
    assert call(handle, 65537) != 0 and call(handle, 1, cover=-1.0) != 0 and call(handle, 1, cover=float("nan")) != 0
    assert call(handle, 1, source=(None,) * 6) != 0 and call(handle, 1, source=(None, None, None, off.data_ptr(), pts.data_ptr(), None)) != 0
    assert call(handle, 1, o=[None] + ptrs[1:]) != 0 and call(handle, 1, o=ptrs[:-1] + [None]) != 0
    assert call(handle, 0, o=[None] * 10) == 0  # n = 0 succeeds and writes nothing
    assert call(handle, 1) == 0
    torch.cuda.synchronize()
    assert int(outs[-1].cpu()[0]) == 0 and int(outs[2].cpu()[0, 0]) == 0 and int(outs[2].cpu()[0, 3]) == 2
    assert lib.pmx_colour_ref_destroy(handle) == 0 and lib.pmx_colour_ref_destroy(None) == 0
    # the Python layer
    ref = case_ref("f63")
    c = combo_cases.case("f63")
    library, _ = combo_cases.library("f63")
    empty = colour(ref, rotation=np.zeros((0, 3, 3)), translation=np.zeros((0, 3)), features=[], feature_types=[])
    assert len(empty) == 0 and empty.type_overlap.shape == (0, 7) and empty.matched_fingerprint.shape == (0, 4)
    assert len(colour(ref, library, [], [], np.zeros((0, 3, 3)), np.zeros((0, 3)))) == 0
    with pytest.raises(ValueError):
        colour(ref, library, [0], [1], [EYE], [ZERO], features=[c["nodes"][0]], feature_types=[c["masks"][0]])
    with pytest.raises(ValueError):
        colour(ref, rotation=[EYE], translation=[ZERO], features=[c["nodes"][3]])
    with pytest.raises(ValueError):
        colour(ref, rotation=[EYE], translation=[ZERO], features=[c["nodes"][3]], feature_types=[c["masks"][4]])
    with pytest.raises(ValueError):
        colour(ref, rotation=[EYE], translation=[ZERO], features=[c["nodes"][3]], feature_types=[c["masks"][3]], cover=-1.0)
    with pytest.raises(ValueError):
        colour(ref, rotation=np.zeros((65537, 3, 3)), translation=np.zeros((65537, 3)), features=[np.zeros((0, 3))] * 65537, feature_types=[[]] * 65537)
    from pharmaconet_amd.shape import ReferenceLigand

    with pytest.raises(ValueError, match="typed features"):
        colour(ReferenceLigand.from_arrays(np.zeros((1, 3)), [1.0]), library, [0], [1], [EYE], [ZERO])
    assert device_colour_ref(ref).self_overlap == result("f63").reference_overlap[0]


# ---------------------------------------------------------------------------------------------------------------- 4. the Python layer
def test_the_report_clusters_hits_by_the_interactions_they_reproduce():
    name = "f63"
    out = result(name)
    sim = out.similarity()
    fp = out.matched_fingerprint[:, 0]
    want = np.array([[1.0 if (a | b) == 0 else bin(int(a & b)).count("1") / bin(int(a | b)).count("1") for b in fp] for a in fp], np.float32)
    assert sim.shape == (64, 64) and np.array_equal(sim, want)
    leaders, leader_of = out.leaders(threshold=0.5)
    assert leaders[0] == 0 and len(leader_of) == 64 and (leader_of[leaders] == leaders).all() and all(sim[i, leader_of[i]] >= 0.5 for i in range(64) if leader_of[i] >= 0)
    popcount = np.array([bin(int(v)).count("1") for v in fp])
    assert np.array_equal(popcount, out.n_reference_matched)


def test_posed_rows_and_the_reference_ligand_carry_the_colour():
    from pharmaconet_amd.engine import Alignment, colour, colour_of
    from pharmaconet_amd.shape import ReferenceLigand

    name = "f63"
    c = combo_cases.case(name)
    lib, conf = combo_cases.library(name)
    n = 8
    al = Alignment(indices=np.arange(n), conformers=conf[:n], rotation=c["R"][:n], translation=c["t"][:n], rmsd=None, rmsd_nodes=None, weight=None, sse=None, scale=None, gap=None,
                   node=None, n_nodes=None, n_pairs=None, levels=None, status=np.zeros(n, np.int32))
    whole = ReferenceLigand.from_arrays(c["ref_xyz"], c["ref_radius"])
    whole.colour = case_ref(name)
    assert same_bits(colour_of(al, whole, lib, cover=COVER), result(name), rows=np.arange(n))
    assert same_bits(colour(whole, lib, np.arange(n), conf[:n], c["R"][:n], c["t"][:n], cover=COVER), result(name), rows=np.arange(n))
