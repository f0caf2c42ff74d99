"""`pmx_pose_refine` without a GPU: the NumPy restatement (tests/refine_ref.py) against what the header promises of the algorithm - the
gradient, the monotone energy, the rows that must come back unchanged, a closed form, the crystal ligand of the 6OIM fixture - and the
sensitivity figure S over exactly the seeded rows of the GPU tests (tests/refine_cases.py), from which their bars follow."""

import numpy as np
import pytest

import clash_ref
import refine_cases
import refine_ref
from conftest import GOLDEN, load_golden
from pharmaconet_amd.pocket import PocketAtoms, element_radii, parse_pdb_atoms


def moved(R, t, c, delta):
    """The trial motion of the header: R' = Rd R, t' = Rd (t - c) + c + tau."""
    Rd = refine_ref.rodrigues(np.asarray(delta[:3], dtype=np.float64))
    return Rd @ R, Rd @ (t - c) + c + np.asarray(delta[3:], dtype=np.float64)


def clashing_rows(count=12):
    """Rows of the "anchors_tw" case (explicit anchors with targets and weights) and of "radii" (own points) that clash at the start."""
    out = []
    for name in ("anchors_tw", "radii"):
        c = refine_cases.case(name)
        ref = refine_cases.reference(name)
        rows = [i for i in range(c["n"]) if ref[i]["energy"][0] > 0][: count // 2]
        out += [(c, i) for i in rows]
    assert len(out) == count
    return out


def make_row(c, i):
    pick = lambda v: None if v is None else v[i]  # noqa: E731
    return refine_ref.Row(c["atom_xyz"], c["atom_radius"], c["points"][i], c["radii"][i] if c["radii"] is not None else np.float32(refine_cases.NODE_RADIUS),
                          pick(c["anchors"]), pick(c["targets"]), pick(c["weights"]), c["R"][i], c["t"][i], refine_cases.TOLERANCE, refine_cases.RESTRAINT)


def test_gradient_against_central_differences():
    """g = grad(E / 2) in the six parameters (omega about the centroid, tau). E is a sum of squares with continuous first derivatives
    (pen^2 enters at pen = 0 with slope 0), so central differences of step h = 1e-6 are off by h^2 |E'''| / 6 + eps E / h: about 1e-9 for
    E of the order of 10. The bar is 1e-6 (1 + |g|)."""
    h, worst = 1e-6, 0.0
    for c, i in clashing_rows():
        row = make_row(c, i)
        R, t = c["R"][i], c["t"][i]
        H, g, cen = refine_ref.normal_equations(row, R, t)
        fd = np.zeros(6)
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            fd[k] = (refine_ref.energy(row, *moved(R, t, cen, d)) - refine_ref.energy(row, *moved(R, t, cen, -d))) / (4.0 * h)
        worst = max(worst, float(np.abs(fd - g).max() / (1.0 + np.abs(g).max())))
        assert np.abs(fd - g).max() <= 1e-6 * (1.0 + np.abs(g).max()), (c["name"], i, fd, g)
        assert np.allclose(H, H.T) and np.linalg.eigvalsh(H).min() >= -1e-9 * np.abs(H).max()  # (J^T J)
    print(f"gradient against central differences: worst {worst:.3e} (bar 1e-6)")


def test_energy_never_rises_over_accepted_steps():
    for c, i in clashing_rows():
        trace = []
        out = refine_cases.reference_row(c, i, trace=trace)
        E = np.array(trace)
        assert len(E) == out["count"][1] + 1 and (np.diff(E) < 0).all()
        assert out["energy"][2] + refine_cases.RESTRAINT * out["energy"][3] == E[-1] <= E[0] == out["energy"][0] + refine_cases.RESTRAINT * out["energy"][1]


def test_clean_rows_and_max_iter_zero_return_their_input():
    c = refine_cases.case("points")
    ref = refine_cases.reference("points")
    clean = [i for i in range(c["n"]) if ref[i]["energy"][0] == 0]
    assert len(clean) >= 8 and len(clean) < c["n"]
    for i in clean:
        r = ref[i]
        assert r["count"].tolist() == [0, 0, 0, 0] and r["status"] == 0
        assert np.array_equal(r["rotation"], c["R"][i]) and np.array_equal(r["translation"], c["t"][i])
        assert r["energy"][[0, 2, 3, 4, 5, 6]].tolist() == [0.0] * 6
    for i in range(16):
        r = refine_cases.reference_row(c, i, max_iter=0)
        assert np.array_equal(r["rotation"], c["R"][i]) and np.array_equal(r["translation"], c["t"][i])
        assert r["count"][:2].tolist() == [0, 0] and r["count"][2] == (0 if ref[i]["energy"][0] == 0 else 2)
        assert r["energy"][0] == r["energy"][2] == ref[i]["energy"][0] and r["count"][3] == (0 if ref[i]["energy"][0] == 0 else r["count"][3])
        assert r["energy"][5] == 0.0 and r["energy"][6] == 0.0


@pytest.mark.parametrize("restraint", [0.1, 1.0, 0.01])
def test_closed_form_of_one_point_against_one_atom(restraint):
    """One point, its own anchor of weight 1, on the x axis at d0 from one atom: E(d) = (s - d)^2 + restraint (d - d0)^2 has its minimum at
    d* = (s + restraint d0) / (1 + restraint). The residuals are linear along the axis, so a damped step of lambda leaves lambda / (1 + lambda)
    <= 1e-3 of the error: at ftol = 0 and 64 iterations the final distance is d* within 1e-6 A."""
    ra, rp, tol, d0 = np.float32(1.7), np.float32(1.25), np.float32(0.5), 1.5
    s = (float(ra) + float(rp)) - float(tol)
    out = refine_ref.refine_row([[0, 0, 0]], [ra], [[d0, 0, 0]], rp, np.eye(3), np.zeros(3), tolerance=tol, restraint=restraint, ftol=0.0, max_iter=64)
    p = clash_ref.pose([[d0, 0, 0]], out["rotation"], out["translation"])[0]
    want = (s + restraint * d0) / (1.0 + restraint)
    print(f"closed form, restraint {restraint}: d {np.linalg.norm(p)!r} against {want!r}, {out['count'].tolist()}")
    assert out["status"] == 0 and abs(np.linalg.norm(p) - want) <= 1e-6 and abs(p[1]) <= 1e-12 and abs(p[2]) <= 1e-12
    assert out["count"][1] >= 2 and out["count"][3] == 1
    assert abs(out["energy"][2] - (s - want) ** 2) <= 1e-6 and abs(out["energy"][4] - (want - d0)) <= 1e-6


def test_crystal_ligand_of_6oim():
    """The bound pose clashes only at its covalent attachment to CYS 12 (tests/test_clash_cpu.py): that pair cannot be relieved, and the
    restraint must win - the pose stays within 0.5 A. Shifted by 1 A along any axis it clashes elsewhere; the refinement lowers that overlap and stays within 1 A."""
    model, _, _, _ = load_golden("set_6oim_c8")
    pocket = PocketAtoms.from_pdb(GOLDEN / "pocket_6oim.pdb", centers=model.node_centers)
    lig = parse_pdb_atoms((GOLDEN / "ligand_6oim_mov.pdb").read_text())
    radii = element_radii(lig.element)
    still = refine_ref.refine_row(pocket.xyz, pocket.radius, lig.xyz, radii, np.eye(3), np.zeros(3))
    print("crystal ligand, unmoved:", still["energy"].tolist(), still["count"].tolist())
    assert still["status"] == 0 and abs(still["energy"][0] - 1.4930) < 5e-5 and still["energy"][2] <= still["energy"][0] and still["energy"][4] < 0.5
    for axis in range(3):
        t = np.zeros(3)
        t[axis] = 1.0
        out = refine_ref.refine_row(pocket.xyz, pocket.radius, lig.xyz, radii, np.eye(3), t)
        print(f"crystal ligand, shifted by 1 A along axis {axis}:", out["energy"].tolist(), out["count"].tolist())
        assert out["status"] == 0 and out["energy"][0] > 0 and out["energy"][2] < out["energy"][0] and out["energy"][4] < 1.0


def test_statuses_of_the_restatement():
    bad = np.eye(3)
    bad[0, 1] = np.nan
    for out in (refine_ref.refine_row([[0, 0, 0]], [1.7], [[1, 0, 0]], 1.0, bad, np.zeros(3)),
                refine_ref.refine_row([[0, 0, 0]], [1.7], [[1, 0, 0]], 1.0, np.eye(3), np.zeros(3), anchors=[[0, 0, 0]], weights=[-1.0]),
                refine_ref.refine_row([[0, 0, 0]], [1.7], [[1, 0, 0]], 1.0, np.eye(3), np.zeros(3), anchors=[[0, 0, 0]], weights=[np.inf])):
        assert out["status"] == 4 and np.isnan(out["rotation"]).all() and np.isnan(out["energy"]).all() and out["count"].tolist() == [0, 0, -1, 0]


def test_sensitivity_over_the_rows_of_the_gpu_tests():
    """S: over every seeded row the GPU tests use, the largest difference between the three variants of the restatement in posed point
    coordinates and in relative final E. All three must agree in every integer on every row, and no row may stand within 1e-9 of a
    decision: the seeds of tests/refine_cases.py are chosen so. The recorded figures (refine_cases.S, one per case) are what the bars of
    the GPU tests are made of, so no case's measured one may exceed its record."""
    worst_p = worst_e = 0.0
    for name in refine_cases.CASES:
        s_pts, s_e, agree, margin = refine_cases.sensitivity(name)
        ref = refine_cases.reference(name)
        stops = np.bincount(np.array([r["count"][2] for r in ref]) + 1, minlength=5).tolist()
        print(f"{name}: S points {s_pts:.3e} A, S energy {s_e:.3e}, decision margin {margin:.3e}, stops (-1, 0, 1, 2, 3) {stops}")
        assert agree, name
        assert margin >= refine_cases.MARGIN, (name, margin)
        assert max(s_pts, s_e) <= refine_cases.S[name], (name, s_pts, s_e, refine_cases.S[name])
        worst_p, worst_e = max(worst_p, s_pts), max(worst_e, s_e)
    print(f"S = {max(worst_p, worst_e):.3e} over all cases (points {worst_p:.3e} A, energy {worst_e:.3e})")
    # the cases cover what they are there for
    started = sum(int(r["energy"][0] > 0) for name in refine_cases.CASES for r in refine_cases.reference(name))
    assert started >= 300
    for name, reasons in (("points", {0, 1}), ("pocket64", {0, 1, 2}), ("iter0", {0, 2}), ("iter1", {0, 2})):
        assert reasons <= {int(r["count"][2]) for r in refine_cases.reference(name)}, name
