"""The NumPy restatement of `pmx_pose_shape` (tests/shape_ref.py) against closed forms and the three exact consequences of include/pmx.h,
`shape.ReferenceLigand`, the margins of every seeded case the GPU tests use, and the argument errors. No GPU."""

import numpy as np
import pytest

import shape_ref
from conftest import GOLDEN

EYE, ZERO = np.eye(3), np.zeros(3)


def golden_reference():
    from pharmaconet_amd.shape import ReferenceLigand

    return ReferenceLigand.from_pdb(GOLDEN / "ligand_6oim_mov.pdb")


def prefactor(ra, rb):
    aa, ab = shape_ref.KAPPA / (float(np.float32(ra)) ** 2), shape_ref.KAPPA / (float(np.float32(rb)) ** 2)
    q = shape_ref.PI / (aa + ab)
    return 8.0 * (q * np.sqrt(q)), (aa * ab) / (aa + ab)


def test_one_atom_on_one_atom_is_the_prefactor():
    """Consequence (ii): d2 = 0, so the term is exactly 8.0 * (q * sqrt(q)); with equal radii every overlap is that number."""
    y = np.array([[1.5, -2.25, 3.0]], np.float32)
    r = shape_ref.shape_row(y, [1.7], y, [1.55], EYE, ZERO)
    pre, _ = prefactor(1.55, 1.7)
    assert r["summary"][0] == pre and r["counts"].tolist() == [1, 1, 1, 1] and r["point_near"][0] == 0.0 and r["ref_near"][0] == 0.0
    same = shape_ref.shape_row(y, [1.7], y, [1.7], EYE, ZERO)
    assert same["summary"][0] == same["summary"][1] == same["summary"][2] == prefactor(1.7, 1.7)[0] and same["summary"][3] == 1.0 and same["summary"][8] == 0.0
    # KAPPA is the one at which an atom's Gaussian of amplitude 2 sqrt 2 integrates to the sphere's volume 4/3 pi r^3
    assert abs(2.0 * np.sqrt(2.0) * (shape_ref.PI / (shape_ref.KAPPA / 1.7**2)) ** 1.5 - 4.0 / 3.0 * np.pi * 1.7**3) < 1e-12 * 30


def test_two_atoms_at_a_distance_by_hand():
    d = 1.25  # (exact in float32, as are the coordinates)
    y = np.array([[0, 0, 0]], np.float32)
    x = np.array([[0, d, 0], [0, 0, -2 * d]], np.float32)
    r = shape_ref.shape_row(y, [1.8], x, [1.52, 1.7], EYE, ZERO, cover=2.0)
    p0, k0 = prefactor(1.52, 1.8)
    p1, k1 = prefactor(1.7, 1.8)
    want = p0 * np.exp(-(k0 * d * d)) + p1 * np.exp(-(k1 * 4 * d * d))
    assert r["summary"][0] == want
    pa, _ = prefactor(1.52, 1.52)
    pb, _ = prefactor(1.7, 1.7)
    pab, kab = prefactor(1.52, 1.7)
    cross = pab * np.exp(-(kab * (5 * d * d)))  # (the two points are d and 2 d out on two axes: d^2 + (2 d)^2 apart)
    assert r["summary"][1] == (pa + cross) + (cross + pb)
    assert r["point_near"].tolist() == [d, 2 * d] and r["point_ref"].tolist() == [0, 0] and r["ref_near"].tolist() == [d] and r["ref_point"].tolist() == [0]
    assert r["counts"].tolist() == [2, 1, 1, 1]  # (2 d = 2.5 is not within the cover of 2)
    assert r["summary"][6] == np.sqrt((d * d + 4 * d * d) / 2.0) and r["summary"][7] == d and np.isnan(r["summary"][8])
    assert r["summary"][3] == r["summary"][0] / ((r["summary"][1] + r["summary"][2]) - r["summary"][0])


def test_golden_ligand_in_place_far_away_and_shifted():
    ref = golden_reference()
    assert len(ref) == 41 and ref.xyz.dtype == np.float32 and ref.radius.dtype == np.float32 and ref.xyz.shape == (41, 3)
    o_bb = shape_ref.self_overlap(ref.xyz, ref.radius)
    assert abs(o_bb - 1755.6669180579565) <= 1e-12 * 1755.6669180579565
    # (i): the reference's own atoms in place
    r = shape_ref.shape_row(ref.xyz, ref.radius, ref.xyz, ref.radius, EYE, ZERO)
    s = r["summary"]
    assert s[0] == s[1] == s[2] == o_bb and s[3] == 1.0 and s[4] == 1.0 and s[5] == 1.0 and s[6] == 0.0 and s[7] == 0.0 and s[8] == 0.0
    assert not r["point_near"].any() and not r["ref_near"].any() and np.array_equal(r["point_ref"], np.arange(41)) and np.array_equal(r["ref_point"], np.arange(41))
    assert r["counts"].tolist() == [41, 41, 41, 41]
    # (iii): far away the overlap underflows to 0
    far = shape_ref.shape_row(ref.xyz, ref.radius, ref.xyz, ref.radius, EYE, [200.0, 0.0, 0.0])
    assert far["summary"][0] == 0.0 and far["summary"][3] == 0.0 and far["summary"][4] == 0.0 and far["summary"][1] == o_bb and far["counts"].tolist() == [41, 0, 0, 41]
    # shifted by 1 A along x (the motion's translation: the posed point is x + 1 in float64)
    moved = shape_ref.shape_row(ref.xyz, ref.radius, ref.xyz, ref.radius, EYE, [1.0, 0.0, 0.0])
    assert abs(moved["summary"][3] - 0.7529757444805636) <= 1e-12
    assert abs(moved["summary"][8] - 1.0) <= 1e-12 and moved["summary"][6] <= 1.0


def test_rows_that_are_not_ok_and_the_empty_row():
    ref = golden_reference()
    bad = EYE.copy()
    bad[0, 1] = np.inf
    pts = np.zeros((3, 3), np.float32)
    for r in (shape_ref.shape_row(ref.xyz, ref.radius, pts, np.float32(1.0), bad, ZERO), shape_ref.shape_row(ref.xyz, ref.radius, pts, [1.0, 0.0, 1.0], EYE, ZERO),
              shape_ref.shape_row(ref.xyz, ref.radius, pts, np.float32(np.nan), EYE, ZERO), shape_ref.shape_row(ref.xyz, ref.radius, pts, [1.0, 1.0, -1.0], EYE, ZERO)):
        assert r["status"] == 4 and np.isnan(r["summary"]).all() and not r["counts"].any() and np.isnan(r["point_near"]).all() and (r["point_ref"] == -1).all()
        assert np.isnan(r["ref_near"]).all() and (r["ref_point"] == -1).all() and len(r["ref_near"]) == 41
    big = shape_ref.shape_row(ref.xyz, ref.radius, np.zeros((257, 3), np.float32), np.float32(1.0), EYE, ZERO)
    assert big["status"] == 1 and len(big["point_near"]) == 257
    empty = shape_ref.shape_row(ref.xyz, ref.radius, np.zeros((0, 3), np.float32), np.float32(np.nan), EYE, ZERO)  # (no point: no bad radius)
    s = empty["summary"]
    assert empty["status"] == 0 and s[0] == 0.0 and s[1] == 0.0 and s[3] == 0.0 and s[4] == 0.0 and s[5] == 0.0 and np.isnan(s[6]) and np.isposinf(s[7]) and np.isnan(s[8])
    assert empty["counts"].tolist() == [0, 0, 0, 41] and np.isposinf(empty["ref_near"]).all() and (empty["ref_point"] == -1).all()


@pytest.mark.parametrize("with_radii", [True, False])
@pytest.mark.parametrize("m", shape_ref.REF_SIZES)
def test_every_seeded_case_of_the_gpu_tests_has_its_margin(m, with_radii):
    *_, rows = shape_ref.gpu_case(m, with_radii)
    assert sorted(int(r["counts"][0]) for r in rows) == sorted(shape_ref.POINT_COUNTS + shape_ref.EXTRA_COUNTS)
    assert all(r["status"] == 0 for r in rows) and min(r["margin"] for r in rows) >= 1e-9
    if m >= 63:
        assert any(r["summary"][3] > 0.1 for r in rows) and any(0 < r["counts"][1] < r["counts"][0] for r in rows)  # (the rows overlap the reference, and not fully)


def test_reference_ligand_constructors_and_their_errors():
    from pharmaconet_amd.pocket import atomic_number_radii
    from pharmaconet_amd.shape import ReferenceLigand

    ref = golden_reference()
    text = (GOLDEN / "ligand_6oim_mov.pdb").read_text()
    assert np.array_equal(ReferenceLigand.from_pdb(text).xyz, ref.xyz) and len(ReferenceLigand.from_pdb(text, resname="MOV")) == 41
    assert set(np.unique(ref.radius)) <= {np.float32(v) for v in (1.7, 1.55, 1.52, 1.47, 1.75, 1.8)}
    with pytest.raises(ValueError):
        ReferenceLigand.from_pdb(text, resname="XYZ")
    by_z = ReferenceLigand.from_elements([[0, 0, 0], [1, 0, 0]], [6, 8])
    assert np.array_equal(by_z.radius, atomic_number_radii([6, 8])) and by_z.xyz.shape == (2, 3)
    for xyz, radius in (([[0, 0, 0]], [1.0, 1.0]), (np.zeros((0, 3)), []), (np.zeros((257, 3)), np.ones(257)), ([[np.nan, 0, 0]], [1.0]), ([[0, 0, 0]], [0.0]),
                        ([[0, 0, 0]], [-1.0]), ([[0, 0, 0]], [np.inf])):
        with pytest.raises(ValueError):
            ReferenceLigand.from_arrays(xyz, radius)
    assert len(ReferenceLigand.from_arrays(np.zeros((256, 3)), np.ones(256))) == 256
    # from_pose: the posed point in float64, rounded to float32 once
    rng = np.random.default_rng(4)
    R, t = shape_ref.random_rotations(rng, 1)[0], rng.uniform(-3, 3, size=3)
    posed = ReferenceLigand.from_pose(ref.xyz, ref.radius, R, t)
    assert np.array_equal(posed.xyz, shape_ref.pose(ref.xyz, R, t).astype(np.float32)) and np.array_equal(posed.radius, ref.radius)
    assert np.array_equal(ReferenceLigand.from_pose(ref.xyz, ref.radius, EYE, ZERO).xyz, ref.xyz)


def test_cli_refuses_pose_shape_without_a_reference(tmp_path, capsys):
    from pharmaconet_amd.screening import main

    base = ["-p", str(GOLDEN / "model_6oim_like.pm"), "-d", str(GOLDEN / "set_6oim_c8.pmxlib"), "-o", str(tmp_path / "x.csv")]
    for bad, word in ((["--explain", "3", "--pose_shape", str(tmp_path / "s.csv")], "--shape_ref"),
                      (["--pose_shape", str(tmp_path / "s.csv"), "--shape_ref", str(GOLDEN / "ligand_6oim_mov.pdb")], "--explain"),
                      (["--explain", "3", "--shape_ref", str(GOLDEN / "ligand_6oim_mov.pdb")], "--pose_shape"),
                      (["--explain", "3", "--pose_shape", str(tmp_path / "s.csv"), "--shape_ref", str(GOLDEN / "ligand_6oim_mov.pdb")], "--shape_level nodes"),  # no .atoms file
                      (["--explain", "3", "--pose_shape", str(tmp_path / "s.csv"), "--shape_ref", str(GOLDEN / "ligand_6oim_mov.pdb"), "--shape_level", "nodes", "--shape_cover", "-1"],
                       "--shape_cover")):
        with pytest.raises(SystemExit):
            main(base + bad)
        assert word in capsys.readouterr().err
    assert not (tmp_path / "x.csv").exists() and not (tmp_path / "s.csv").exists()
