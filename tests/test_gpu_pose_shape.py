"""`pmx_pose_shape` on the GPU (csrc/pmx_pose_shape.hip) against the NumPy restatement of tests/shape_ref.py: point mode over the shapes at
which the kernel's trips change, node mode on the golden sets' own poses, the atom store against host points, the three exact consequences
of include/pmx.h, rows that are not OK, the host's checks, repeatability, and the Python layer and the command line on top of it.

Bars. Statuses, counts and the four index outputs must be equal: they depend on correctly rounded operations alone, and
tests/test_shape_cpu.py shows every seeded case to stand at least 1e-9 off every place where one could differ (the `margin`, asserted
again here: no row is skipped for it). Distances: 1e-12 * max(1, |v|). Overlaps: 1e-13 * v + 1e-300 - sums of at most 256 * 512
non-negative terms in the restatement's own order, each term differing by the two `exp` implementations alone (an ulp or two, 2e-16
relative each; the bar and the argument of tests/test_gpu_pose_fit.py). The three ratios are asserted to be exactly the header's formulas
applied in NumPy to the device's own three overlaps; the three RMS values come from sums without an `exp`, which the restatement forms
bit for bit as the device does, so they are asserted equal to the restatement's."""

import ctypes
from functools import lru_cache

import numpy as np
import pytest

import shape_ref
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

MARGIN = 1e-9
K_WAVES = 4  # rows per block of shape_kernel
EYE, ZERO = np.eye(3), np.zeros(3)
FIELDS = ("overlap", "self_overlap", "reference_overlap", "tanimoto", "reference_fraction", "fit_fraction", "rms_to_reference", "rms_from_reference", "rmsd_in_order",
          "n_points", "n_covered", "n_reference_covered", "status")
LISTS = ("point_distance", "point_reference_atom", "reference_distance", "reference_point")


@lru_cache(maxsize=None)
def golden_reference():
    from pharmaconet_amd.shape import ReferenceLigand

    return ReferenceLigand.from_pdb(GOLDEN / "ligand_6oim_mov.pdb")


def close(got, want, rel):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    fin = np.isfinite(want)
    return np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]) and bool((np.abs(got[fin] - want[fin]) <= rel * np.maximum(1.0, np.abs(want[fin]))).all())


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def check_report(rep, ref, tag):
    """Every row of `rep` against the restatement's rows `ref`; the figures are printed before they are asserted."""
    assert len(rep) == len(ref), tag
    margin = min([r["margin"] for r in ref], default=np.inf)
    worst_d = worst_o = 0.0
    for i, r in enumerate(ref):
        if r["status"] != 0:
            continue
        for got, want in ((rep.point_distance[i], r["point_near"]), (rep.reference_distance[i], r["ref_near"])):
            fin = np.isfinite(want)
            if fin.any():
                worst_d = max(worst_d, float((np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))).max()))
        for got, want in ((rep.overlap[i], r["summary"][0]), (rep.self_overlap[i], r["summary"][1]), (rep.reference_overlap[i], r["summary"][2])):
            if want > 0:
                worst_o = max(worst_o, abs(got - want) / want)
    print(f"{tag}: rows {len(ref)} margin {margin:.3e} worst distance error {worst_d:.3e} (bar 1e-12) worst overlap error {worst_o:.3e} (bar 1e-13)")
    assert margin >= MARGIN, (tag, margin)
    for i, r in enumerate(ref):
        where = (tag, i)
        assert rep.status[i] == r["status"], where
        got = [int(rep.n_points[i]), int(rep.n_covered[i]), int(rep.n_reference_covered[i])]
        assert got == r["counts"][:3].tolist(), (where, got, r["counts"])
        assert np.array_equal(rep.point_reference_atom[i], r["point_ref"]) and np.array_equal(rep.reference_point[i], r["ref_point"]), where
        assert close(rep.point_distance[i], r["point_near"], 1e-12) and close(rep.reference_distance[i], r["ref_near"], 1e-12), where
        dev = np.array([rep.overlap[i], rep.self_overlap[i], rep.reference_overlap[i], rep.tanimoto[i], rep.reference_fraction[i], rep.fit_fraction[i],
                        rep.rms_to_reference[i], rep.rms_from_reference[i], rep.rmsd_in_order[i]])
        if r["status"] != 0:
            assert np.isnan(dev).all(), where
            continue
        for k in range(3):
            assert abs(dev[k] - r["summary"][k]) <= 1e-13 * r["summary"][k] + 1e-300, (where, k, dev[k], r["summary"][k])
        _, _, s_a, s_b, s_o = r["sums"]
        want = shape_ref.ratios(dev[0], dev[1], dev[2], s_a, s_b, s_o, int(r["counts"][0]), int(r["counts"][3]))
        assert same(dev[3:9], want[3:9]), (where, dev[3:9], want[3:9])


def same_bits(a, b, rows=None):
    """Report `a` equals report `b` (its rows `rows`) bit for bit."""
    rows = np.arange(len(b)) if rows is None else np.asarray(rows)
    return (len(a) == len(rows) and all(same(getattr(a, f), getattr(b, f)[rows]) for f in FIELDS)
            and all(same(getattr(a, f)[k], getattr(b, f)[j]) for f in LISTS for k, j in enumerate(rows)))


def not_ok_fill(rep, i, n_points, m):
    return (np.isnan([getattr(rep, f)[i] for f in FIELDS[:9]]).all() and (rep.n_points[i], rep.n_covered[i], rep.n_reference_covered[i]) == (0, 0, 0)
            and len(rep.point_distance[i]) == n_points and np.isnan(rep.point_distance[i]).all() and (rep.point_reference_atom[i] == -1).all()
            and len(rep.reference_distance[i]) == m and np.isnan(rep.reference_distance[i]).all() and (rep.reference_point[i] == -1).all())


def case_reference(m, with_radii=True):
    from pharmaconet_amd.shape import ReferenceLigand

    ref_xyz, ref_radius, points, radii, R, t, rows = shape_ref.gpu_case(m, with_radii)
    return ReferenceLigand.from_arrays(ref_xyz, ref_radius), points, radii, R, t, rows


# ---------------------------------------------------------------------------------------------------------------- 1. point mode
@pytest.mark.parametrize("with_radii", [True, False])
@pytest.mark.parametrize("m", shape_ref.REF_SIZES)
def test_point_mode_against_the_restatement(m, with_radii):
    from pharmaconet_amd.engine import device_shape_ref, shape

    ref, points, radii, R, t, rows = case_reference(m, with_radii)
    rep = shape(ref, rotation=R, translation=t, points=points, point_radii=radii, node_radius=float(shape_ref.NODE_RADIUS), cover=shape_ref.COVER)
    check_report(rep, rows, f"points, reference of {m}, radii {with_radii}")
    assert set(shape_ref.POINT_COUNTS) <= set(int(v) for v in rep.n_points)
    assert (rep.reference_overlap == device_shape_ref(ref).self_overlap).all()
    # (the reference as a row of its own, in place: O_AA is O_BB bit for bit at every size)
    own = shape(ref, rotation=[EYE], translation=[ZERO], points=[ref.xyz], point_radii=[ref.radius])
    assert own.self_overlap[0] == own.reference_overlap[0] == own.overlap[0] and own.tanimoto[0] == 1.0


@pytest.mark.parametrize("n", [1, K_WAVES - 1, K_WAVES, K_WAVES + 1])
def test_the_tail_of_the_last_block(n):
    from pharmaconet_amd.engine import shape

    ref, points, radii, R, t, rows = case_reference(65)
    pick = [7, 2, 12, 5, 0][:n]  # (256 points first: the longest row of the call stands in wave 0)
    rep = shape(ref, rotation=R[pick], translation=t[pick], points=[points[j] for j in pick], point_radii=[radii[j] for j in pick], cover=shape_ref.COVER)
    check_report(rep, [rows[j] for j in pick], f"a call of {n} rows")


# ---------------------------------------------------------------------------------------------------------------- 2. node mode
@pytest.mark.parametrize("name", ["set_6oim_c8", "set_6oim_c64"])
def test_node_mode_at_the_first_and_the_last_conformer(name):
    from pharmaconet_amd.engine import shape
    from test_gpu_align import posed

    model, lib, weights, ex, al = posed(name)
    ref = golden_reference()
    o_bb = shape_ref.self_overlap(ref.xyz, ref.radius)
    heads = lib.headers()
    assert (al.status == 0).sum() >= 16
    for which in ("first", "last"):
        conf = np.array([0 if which == "first" else int(heads[int(i), 1]) - 1 for i in al.indices])
        rep = shape(ref, library=lib, indices=al.indices, conformers=conf, rotation=al.rotation, translation=al.translation, node_radius=1.7, cover=2.0)
        nodes = [lib.unpack(int(i))["xyz"][:, :, int(c)].astype(np.float32) for i, c in zip(al.indices, conf)]
        rows = [shape_ref.shape_row(ref.xyz, ref.radius, nodes[r], np.float32(1.7), al.rotation[r], al.translation[r], 2.0, o_bb=o_bb) for r in range(len(al))]
        check_report(rep, rows, f"nodes, {name}, {which} conformer")
        assert np.array_equal(rep.status == 0, al.status == 0) and (rep.overlap[al.status == 0] > 0).any()  # (the model is in the crystal frame)
        as_points = shape(ref, rotation=al.rotation, translation=al.translation, points=nodes, node_radius=1.7, cover=2.0)
        assert same_bits(as_points, rep)  # the same float32 positions as points: the same bits
    if name == "set_6oim_c64":
        assert int(heads[al.indices.astype(np.int64), 1].max()) == 64


# ---------------------------------------------------------------------------------------------------------------- 3. the atom store
def test_the_atom_store_equals_host_points_bit_for_bit():
    from pharmaconet_amd.atoms import PackedAtoms
    from pharmaconet_amd.engine import DeviceAtoms, shape
    from pharmaconet_amd.pocket import atomic_number_radii
    from test_attribution_cpu import load_mols
    from test_gpu_align import posed

    ref = golden_reference()
    # the golden set's molecules, under their own poses
    model, lib, weights, ex, al = posed("set_6oim_c8")
    mols = load_mols("set_6oim_c8")
    st = PackedAtoms.for_library(mols, lib)
    want = al.shape(ref, atoms=[mols[int(i)] for i in al.indices])
    assert (want.status == 0).sum() >= 16 and (want.n_points[want.status == 0] > 0).all() and (want.overlap[want.status == 0] > 0).any()
    dat = DeviceAtoms(st)
    for source in (st, dat):
        assert same_bits(al.shape(ref, atoms=source), want)
        assert same_bits(shape(ref, atoms=source, indices=al.indices, conformers=al.conformers, rotation=al.rotation, translation=al.translation), want)
    dat.close()
    # a store with a header-only record, and rows that ask for a conformer the record lacks
    rng = np.random.default_rng(12)
    zs = [np.array([1, 1]), rng.choice([6, 7, 8, 16, 17], size=5), rng.choice([6, 7, 8, 9, 35], size=70)]
    ps = [rng.uniform(-4, 4, size=(len(z), 2, 3)).astype(np.float32) for z in zs]
    edge = PackedAtoms.from_arrays(zs, ps)
    lig, conf = [0, 1, 1, 2, 2, 3], [0, 0, 2, 1, -1, 0]
    R, t = shape_ref.random_rotations(rng, 6), rng.uniform(-1, 1, size=(6, 3))
    got = shape(ref, atoms=edge, indices=lig, conformers=conf, rotation=R, translation=t)
    assert got.status.tolist() == [1, 0, 4, 0, 4, 1]
    for i in (0, 2, 4, 5):
        assert not_ok_fill(got, i, 0, 41)
    ok = [1, 3]
    host = shape(ref, rotation=R[ok], translation=t[ok], points=[ps[lig[i]][:, conf[i]] for i in ok], point_radii=[atomic_number_radii(zs[lig[i]]) for i in ok])
    assert same_bits(host, got, rows=ok) and host.n_points.tolist() == [5, 70]
    o_bb = shape_ref.self_overlap(ref.xyz, ref.radius)
    rows = [shape_ref.shape_row(ref.xyz, ref.radius, ps[lig[i]][:, conf[i]], atomic_number_radii(zs[lig[i]]), R[i], t[i], o_bb=o_bb) for i in ok]
    check_report(host, rows, "the edge store's rows")


# ---------------------------------------------------------------------------------------------------------------- 4. the exact consequences
def test_the_three_exact_consequences():
    from pharmaconet_amd.engine import device_shape_ref, shape
    from pharmaconet_amd.shape import ReferenceLigand

    ref = golden_reference()
    o_bb = device_shape_ref(ref).self_overlap
    print(f"O_BB of the golden ligand on the device: {o_bb!r} (the restatement: {shape_ref.self_overlap(ref.xyz, ref.radius)!r})")
    assert abs(o_bb - 1755.6669180579565) <= 1e-12 * 1755.6669180579565
    # (i) the reference's own atoms in place; (iii) the same atoms 200 A away; and 1 A along x
    rep = shape(ref, rotation=[EYE] * 3, translation=[ZERO, [200.0, 0, 0], [1.0, 0, 0]], points=[ref.xyz] * 3, point_radii=[ref.radius] * 3)
    assert rep.overlap[0] == rep.self_overlap[0] == rep.reference_overlap[0] == o_bb and rep.tanimoto[0] == 1.0 and rep.reference_fraction[0] == 1.0 and rep.fit_fraction[0] == 1.0
    assert not rep.point_distance[0].any() and not rep.reference_distance[0].any() and rep.rmsd_in_order[0] == 0.0 and rep.rms_to_reference[0] == 0.0 and rep.rms_from_reference[0] == 0.0
    assert np.array_equal(rep.point_reference_atom[0], np.arange(41)) and np.array_equal(rep.reference_point[0], np.arange(41)) and rep.n_covered[0] == rep.n_reference_covered[0] == 41
    assert rep.overlap[1] == 0.0 and rep.tanimoto[1] == 0.0 and rep.reference_fraction[1] == 0.0 and rep.self_overlap[1] == o_bb and rep.n_covered[1] == 0
    assert abs(rep.tanimoto[2] - 0.7529757444805636) <= 1e-12 and abs(rep.rmsd_in_order[2] - 1.0) <= 1e-12
    # (ii) one point on one reference atom: exactly the prefactor
    one = ReferenceLigand.from_arrays([[1.5, -2.25, 3.0]], [1.7])
    rep = shape(one, rotation=[EYE], translation=[ZERO], points=[one.xyz], point_radii=[[1.55]])
    aa, ab = shape_ref.KAPPA / (float(np.float32(1.55)) ** 2), shape_ref.KAPPA / (float(np.float32(1.7)) ** 2)
    q = shape_ref.PI / (aa + ab)
    assert rep.overlap[0] == 8.0 * (q * np.sqrt(q)) and rep.point_distance[0][0] == 0.0


# ---------------------------------------------------------------------------------------------------------------- 5. rows that are not OK
def test_rows_that_are_not_ok_and_the_empty_row():
    from pharmaconet_amd.engine import align, shape

    model, lib, weights, _ = load_golden("set_6oim_c8")
    ref = golden_reference()
    C, n0 = int(lib.header(0)[1]), int(lib.header(0)[0])
    bad_r, bad_t = EYE.copy(), ZERO.copy()
    bad_r[1, 2], bad_t[0] = np.nan, np.inf
    idx = [len(lib), 0, 0, 0, 0, 0, len(lib) + 10**9]
    conf = [0, C, -1, 0, 0, 0, 0]
    rot = [EYE, EYE, EYE, bad_r, EYE, EYE, EYE]
    trans = [ZERO, ZERO, ZERO, ZERO, bad_t, ZERO, ZERO]
    rep = shape(ref, library=lib, indices=idx, conformers=conf, rotation=rot, translation=trans)
    assert rep.status.tolist() == [1, 4, 4, 4, 4, 0, 1]
    for i in (0, 1, 2, 3, 4, 6):
        assert not_ok_fill(rep, i, 0 if rep.status[i] == 1 else n0, 41), i
    want = shape_ref.shape_row(ref.xyz, ref.radius, lib.unpack(0)["xyz"][:, :, 0], np.float32(1.0), EYE, ZERO)
    assert want["margin"] >= MARGIN
    check_report(shape(ref, library=lib, indices=[0], conformers=[0], rotation=[EYE], translation=[ZERO]), [want], "node mode, one row")
    # a bad radius: the call's own in node mode and in point mode, a point's in point mode
    for radius in (0.0, -1.0):
        nodes = shape(ref, library=lib, indices=[0, len(lib)], conformers=[0, 0], rotation=[EYE, EYE], translation=[ZERO, ZERO], node_radius=radius)
        assert nodes.status.tolist() == [4, 1] and not_ok_fill(nodes, 0, n0, 41)
    pts = [np.zeros((3, 3), np.float32), np.ones((2, 3), np.float32), np.zeros((0, 3), np.float32), np.ones((70, 3), np.float32)]
    radii = [[1.5, np.nan, 1.5], [1.5, 1.5], [], [1.5] * 69 + [0.0]]
    pm = shape(ref, rotation=[EYE] * 4, translation=[ZERO] * 4, points=pts, point_radii=radii)
    assert pm.status.tolist() == [4, 0, 0, 4] and not_ok_fill(pm, 0, 3, 41) and not_ok_fill(pm, 3, 70, 41)
    inf = shape(ref, rotation=[EYE, bad_r], translation=[ZERO, ZERO], points=pts[:2], node_radius=float("-1"))
    assert inf.status.tolist() == [4, 4] and not_ok_fill(inf, 1, 2, 41)
    # a valid empty row in point mode (it has no point, so no radius to be wrong), next to a row with points
    assert pm.status[2] == 0 and pm.n_points[2] == 0 and pm.overlap[2] == 0.0 and pm.self_overlap[2] == 0.0 and pm.tanimoto[2] == 0.0 and pm.fit_fraction[2] == 0.0
    assert np.isnan(pm.rms_to_reference[2]) and np.isposinf(pm.rms_from_reference[2]) and np.isnan(pm.rmsd_in_order[2]) and pm.n_reference_covered[2] == 0
    assert np.isposinf(pm.reference_distance[2]).all() and (pm.reference_point[2] == -1).all() and len(pm.point_distance[2]) == 0
    empty = shape_ref.shape_row(ref.xyz, ref.radius, pts[2], np.float32(1.0), EYE, ZERO)
    check_report(shape(ref, rotation=[EYE], translation=[ZERO], points=[pts[2]]), [empty], "an empty row alone")
    # more points than a row can hold
    big = shape(ref, rotation=[EYE, EYE], translation=[ZERO, ZERO], points=[np.zeros((257, 3), np.float32), pts[1]])
    assert big.status.tolist() == [1, 0] and not_ok_fill(big, 0, 257, 41) and same_bits(shape(ref, rotation=[EYE], translation=[ZERO], points=[pts[1]]), big, rows=[1])
    # a row of an Alignment that is not OK passes through with its status
    al = align(model, lib, [0, 1], [0, C + 3], [[-1], [-1]], weights=weights)
    through = al.shape(ref, lib)
    assert al.status.tolist() == [0, 4] and through.status.tolist() == [0, 4] and np.isnan(through.tanimoto[1])
    # n = 0
    none = shape(ref, library=lib, indices=[], conformers=[], rotation=np.zeros((0, 3, 3)), translation=np.zeros((0, 3)))
    assert len(none) == 0 and none.tanimoto.shape == (0,) and shape(ref, rotation=[], translation=[], points=[]).status.shape == (0,)


# ---------------------------------------------------------------------------------------------------------------- 6. the host's checks
def raw_call(ref, n=1, lib=None, node=False, pts=False, null=(), radius=1.0, cover=2.0):
    """pmx_pose_shape itself with one identity row: `node` / `pts` say which sources are given, `null` which outputs are withheld. The
    return code, the message, and the outputs (filled with a sentinel first: a refused call launches nothing and leaves it)."""
    import torch

    from pharmaconet_amd import _ffi
    from pharmaconet_amd.engine import device_shape_ref

    dev = torch.device("cuda", torch.cuda.current_device())
    rh = device_shape_ref(ref, dev.index)
    lig, conf = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    off, xyz = torch.tensor([0, 1], dtype=torch.int64, device=dev), torch.zeros((1, 3), dtype=torch.float32, device=dev)
    rot, trans = torch.tensor(np.eye(3).reshape(1, 9), device=dev), torch.zeros((1, 3), dtype=torch.float64, device=dev)
    out = dict(summary=torch.full((1, 10), -7.0, dtype=torch.float64, device=dev), count=torch.full((1, 4), -7, dtype=torch.int32, device=dev),
               pnear=torch.full((64,), -7.0, dtype=torch.float64, device=dev), pref=torch.full((64,), -7, dtype=torch.int32, device=dev),
               rnear=torch.full((1, 256), -7.0, dtype=torch.float64, device=dev), rpoint=torch.full((1, 256), -7, dtype=torch.int32, device=dev),
               status=torch.full((1,), -7, dtype=torch.int32, device=dev))
    ptr = {k: (None if k in null else v.data_ptr()) for k, v in out.items()}
    stream = torch.cuda.current_stream(dev)
    lib_ = _ffi.load()
    rc = lib_.pmx_pose_shape(rh.handle, lib.handle if node else None, lig.data_ptr() if node else None, conf.data_ptr() if node else None, off.data_ptr() if pts else None,
                             xyz.data_ptr() if pts else None, None, rot.data_ptr(), trans.data_ptr(), n, radius, cover, ptr["summary"], ptr["count"], ptr["pnear"], ptr["pref"],
                             ptr["rnear"], ptr["rpoint"], ptr["status"], ctypes.c_void_p(stream.cuda_stream))
    message = lib_.pmx_last_error().decode() if rc else ""
    stream.synchronize()
    return rc, message, {k: v.cpu().numpy() for k, v in out.items()}


def untouched(out):
    return all((v == -7).all() for v in out.values())


def test_the_host_refuses_what_the_header_refuses():
    from pharmaconet_amd import _ffi
    from pharmaconet_amd.engine import DeviceLibrary, shape

    lib_ = _ffi.load()
    # the reference: m = 0, m = 257, a NaN coordinate, a bad radius - nothing is made
    xyz, radius = np.zeros((257, 3), np.float32), np.ones(257, np.float32)
    for m, poison in ((0, None), (257, None), (3, "xyz"), (3, "nan radius"), (3, "zero radius")):
        x, r = xyz.copy(), radius.copy()
        if poison == "xyz":
            x[2, 1] = np.nan
        elif poison == "nan radius":
            r[1] = np.inf
        elif poison == "zero radius":
            r[2] = 0.0
        handle = ctypes.c_void_p()
        rc = lib_.pmx_shape_ref_create(x.ctypes.data, r.ctypes.data, m, 0, ctypes.byref(handle))
        assert rc == 1 and not handle.value and b"pmx_shape_ref_create" in lib_.pmx_last_error(), (m, poison)
    assert lib_.pmx_shape_ref_destroy(None) == 0 and lib_.pmx_shape_ref_self(None, None) == 1
    # the call
    _, lib, _, _ = load_golden("set_6oim_c8")
    ref = golden_reference()
    dlib = DeviceLibrary(lib)
    for kw, word in ((dict(lib=dlib, node=True, pts=True), "one source"), (dict(), "neither"), (dict(n=65537, pts=True), "65537"), (dict(pts=True, radius=float("nan")), "finite"),
                     (dict(pts=True, cover=-1.0), "cover"), (dict(pts=True, cover=float("inf")), "cover"), (dict(n=0, lib=dlib, node=True, pts=True), "one source")):
        rc, message, out = raw_call(ref, **kw)
        assert rc == 1 and "pmx_pose_shape" in message and word in message and untouched(out), (kw, message)
    for name in ("summary", "count", "pnear", "pref", "rnear", "rpoint", "status"):
        for kw in (dict(pts=True), dict(lib=dlib, node=True)):
            rc, message, out = raw_call(ref, null=(name,), **kw)
            assert rc == 1 and "null output" in message and untouched(out), (name, message)
    rc, _, out = raw_call(ref, n=0, pts=True)  # n = 0 succeeds and writes nothing
    assert rc == 0 and untouched(out)
    rc, _, out = raw_call(ref, pts=True)
    assert rc == 0 and out["status"][0] == 0 and out["count"][0, 0] == 1 and out["count"][0, 3] == 41 and out["summary"][0, 9] == 0.0 and (out["pnear"][1:] == -7).all()
    assert np.isposinf(out["rnear"][0, 41:]).all() and (out["rpoint"][0, 41:] == -1).all() and (out["rpoint"][0, :41] == 0).all()
    rc, _, out = raw_call(ref, lib=dlib, node=True)
    n0 = int(lib.header(0)[0])
    assert rc == 0 and out["status"][0] == 0 and out["count"][0, 0] == n0 and np.isnan(out["pnear"][n0:]).all() and (out["pref"][n0:] == -1).all()
    dlib.close()
    with pytest.raises(ValueError):
        shape(ref, library=lib, indices=[0], conformers=[0], rotation=[EYE], translation=[ZERO], points=[np.zeros((1, 3))])
    with pytest.raises(ValueError):
        shape(ref, rotation=[EYE], translation=[ZERO])


# ---------------------------------------------------------------------------------------------------------------- 7. repeatability
def test_same_bits_twice_and_under_a_permutation_of_the_rows():
    from pharmaconet_amd.engine import shape

    ref, points, radii, R, t, rows = case_reference(256)
    a = shape(ref, rotation=R, translation=t, points=points, point_radii=radii, cover=shape_ref.COVER)
    b = shape(ref, rotation=R, translation=t, points=points, point_radii=radii, cover=shape_ref.COVER)
    assert same_bits(a, b)
    perm = np.random.default_rng(3).permutation(len(points))
    c = shape(ref, rotation=R[perm], translation=t[perm], points=[points[j] for j in perm], point_radii=[radii[j] for j in perm], cover=shape_ref.COVER)
    assert same_bits(c, a, rows=perm)


# ---------------------------------------------------------------------------------------------------------------- 8. the Python layer
def small_library(lib, k):
    """The k ligands of `lib` with the fewest nodes among those with at least 4, in library order: explaining a hit costs by the size of its
    match tree, and these tests are about what happens after."""
    n_nodes = lib.headers()[:, 0]
    few = np.flatnonzero(n_nodes >= 4)
    return lib.select(np.sort(few[np.argsort(n_nodes[few], kind="stable")[:k]]))


def test_the_methods_agree_with_the_call():
    from pharmaconet_amd.engine import pose_search, shape
    from pharmaconet_amd.shape import ReferenceLigand
    from test_attribution_cpu import load_mols
    from test_gpu_align import posed
    from test_gpu_clash import pocket_6oim

    model, lib, weights, ex, al = posed("set_6oim_c8")
    mols = load_mols("set_6oim_c8")
    ref, pocket = golden_reference(), pocket_6oim()
    nodes = al.shape(ref, lib, cover=2.5)
    assert same_bits(nodes, shape(ref, library=lib, indices=al.indices, conformers=al.conformers, rotation=al.rotation, translation=al.translation, cover=2.5))
    refined = al.refine(pocket, lib)
    assert same_bits(refined.shape(ref, lib), shape(ref, library=lib, indices=al.indices, conformers=al.conformers, rotation=refined.rotation, translation=refined.translation))
    ps = pose_search(model, lib, pocket, list(range(8)), modes=2, weights=weights)
    chosen = ps.alignment()
    assert same_bits(ps.shape(ref, lib), shape(ref, library=lib, indices=chosen.indices, conformers=chosen.conformers, rotation=chosen.rotation, translation=chosen.translation))
    # one ligand: the atoms of a molecule, the nodes of a record; a hit's own pose as the reference
    r = next(r for r in range(len(al)) if al.n_nodes[r] >= 3)
    i = int(al.indices[r])
    atoms = al.shape(ref, atoms=[mols[int(j)] for j in al.indices])
    one = model.scoring_shape(mols[i], ref, weights=weights)
    assert one["level"] == "atoms" and one["status"] == 0 and one["conformer"] == al.conformers[r] and np.array_equal(one["rotation"], al.rotation[r])
    assert (one["overlap"], one["tanimoto"], one["n_points"], one["n_covered"], one["rms_to_reference"]) == (
        atoms.overlap[r], atoms.tanimoto[r], atoms.n_points[r], atoms.n_covered[r], atoms.rms_to_reference[r])
    assert np.array_equal(one["point_distance"], atoms.point_distance[r]) and np.array_equal(one["reference_point"], atoms.reference_point[r])
    packed = model.scoring_shape(lib.record(i), ref, weights=weights)
    assert packed["level"] == "nodes" and packed["n_points"] == nodes.n_points[r] and packed["overlap"] == al.shape(ref, lib).overlap[r]
    again = model.scoring_shape(lib.record(i), ref, weights=weights, refine=True, pocket=pocket)
    assert again["overlap"] == packed["overlap"] and again["refined"]["status"] == 0 and again["refined"]["stop"] >= 0
    z = np.asarray(mols[i].atomic_nums)
    own = ReferenceLigand.from_pose(np.asarray(mols[i].atom_positions, np.float32)[z > 1, int(al.conformers[r])], atoms.point_distance[r] * 0 + 1.7, al.rotation[r], al.translation[r])
    back = shape(own, rotation=[EYE], translation=[ZERO], points=[own.xyz], point_radii=[own.radius])
    assert back.tanimoto[0] == 1.0 and len(own) == atoms.n_points[r]


def test_fitting_with_a_reference_changes_no_other_field():
    import dataclasses

    from test_gpu_clash import pocket_6oim

    model, lib, weights, _ = load_golden("set_6oim_c8")
    ref, pocket = golden_reference(), pocket_6oim()
    lib = small_library(lib, 24)
    res = model.screen(lib, weights=weights)
    for kw in (dict(refine=True, fit=True),):  # (with the refinement: the shape is taken at the motion finally used)
        plain = res.fitting(5, pool=16, max_clashing=2, pocket=pocket, **kw)
        with_shape = res.fitting(5, pool=16, max_clashing=2, pocket=pocket, shape=ref, shape_cover=2.5, **kw)
        assert plain.shape is None and with_shape.shape is not None and len(with_shape.shape) == len(with_shape.poses)
        for f in dataclasses.fields(plain):
            a, b = getattr(plain, f.name), getattr(with_shape, f.name)
            if f.name == "shape" or a is None:
                assert f.name == "shape" or b is None
            elif dataclasses.is_dataclass(a):
                for g in dataclasses.fields(a):
                    x, y = getattr(a, g.name), getattr(b, g.name)
                    assert (all(same(u, v) for u, v in zip(x, y)) and len(x) == len(y)) if isinstance(x, list) else (x is y is None or same(x, y)), (f.name, g.name)
            else:
                assert same(a, b), f.name
        al = with_shape.poses
        assert same_bits(with_shape.shape, al.shape(ref, lib, cover=2.5))  # (at the motion finally used)
    with pytest.raises(ValueError):
        res.fitting(5, pool=16, pocket=pocket, shape_cover=2.5)


def test_cli_pose_shape_csv(tmp_path):
    from pharmaconet_amd.engine import explain
    from pharmaconet_amd.screening import POSE_SHAPE_HEADER, Hits, main, write_pose_shape_csv
    from test_gpu_clash import pocket_6oim

    model, lib, _, _ = load_golden("set_6oim_c8")
    ref, pocket = golden_reference(), pocket_6oim()
    lib = small_library(lib, 12)  # (the command line is what is tested)
    libfile = tmp_path / "lib.pmxlib"
    lib.save(libfile)
    args = ["-p", str(GOLDEN / "model_6oim_like.pm"), "-d", str(libfile), "--explain", "5"]
    side = ["--explain_out", "hits.csv", "--refine_out", "refine.csv", "--protein", str(GOLDEN / "pocket_6oim.pdb"), "--clash_level", "nodes"]
    shape_args = ["--pose_shape", str(tmp_path / "shape.csv"), "--shape_ref", str(GOLDEN / "ligand_6oim_mov.pdb"), "--shape_level", "nodes", "--shape_cover", "2.5"]

    def run(tag, extra):
        (tmp_path / tag).mkdir()
        placed = [str(tmp_path / tag / a) if a.endswith(".csv") else a for a in side]
        main(args + ["-o", str(tmp_path / tag / "main.csv")] + placed + extra)

    run("plain", [])
    run("with", shape_args)
    for name in ("main.csv", "hits.csv", "refine.csv"):  # the main CSV and every other side CSV keep their bytes
        assert (tmp_path / "plain" / name).read_bytes() == (tmp_path / "with" / name).read_bytes(), name
    hits = [row.split(",") for row in (tmp_path / "with" / "hits.csv").read_text().splitlines()[1:]]
    rows = (tmp_path / "shape.csv").read_text().splitlines()
    assert rows[0] == POSE_SHAPE_HEADER == ("rank,path,conformer,stage,level,points,covered,reference_atoms,reference_covered,overlap,tanimoto,reference_fraction,fit_fraction,"
                                            "rms_to_reference,rms_from_reference")
    assert len(rows) == 2 * len(hits) + 1 == 11
    names = {f"{libfile}#{i}": i for i in range(len(lib))}
    idx = [names[h[1]] for h in hits]
    al = explain(model, lib, idx).poses(model, lib)  # (the command line's default weights are the engine's)
    stages = {"fit": al.shape(ref, lib, cover=2.5), "refined": al.refine(pocket, lib, tolerance=0.5, restraint=0.1, max_iter=32).shape(ref, lib, cover=2.5)}
    for k, row in enumerate(rows[1:]):
        f, r = row.split(","), k // 2
        sh = stages[f[3]]
        assert len(f) == 15 and int(f[0]) == r + 1 and f[1] == hits[r][1] and int(f[2]) == int(hits[r][3]) and f[3] == ("fit", "refined")[k % 2] and f[4] == "nodes"
        assert [int(f[5]), int(f[6]), int(f[7]), int(f[8])] == [int(sh.n_points[r]), int(sh.n_covered[r]), 41, int(sh.n_reference_covered[r])]
        want = (sh.overlap[r], sh.tanimoto[r], sh.reference_fraction[r], sh.fit_fraction[r], sh.rms_to_reference[r], sh.rms_from_reference[r])
        assert [float(v) for v in f[9:]] == [float(v) for v in want] and f[9] == repr(float(sh.overlap[r]))
    # without the refinement one row per hit: the writer itself, under scores that rank the same five hits in the same order
    scores = np.zeros(len(lib), np.float32)
    scores[idx] = np.arange(len(idx), 0, -1)
    write_pose_shape_csv(tmp_path / "short.csv", Hits(list(names), scores, np.zeros(len(lib), np.int32), model, lib, None, 5), ref, "nodes", 2.5)
    short = (tmp_path / "short.csv").read_text().splitlines()
    assert len(short) == 6 and short[1:] == rows[1::2]
