"""`pmx_shape_overlay` and `pmx_shape_starts` without a GPU: the NumPy restatement (tests/overlay_ref.py) against what the header promises
of the algorithm - the gradient is the overlap's, the iteration never lowers O_AB and brings a moved copy back, the Jacobi frame is a frame,
one of the four starts finds a turned copy - and the sensitivity figure S over exactly the seeded rows of the GPU tests
(tests/overlay_cases.py), from which their bars follow."""

import ctypes
import re

import numpy as np

import overlay_cases
import overlay_ref
import shape_ref
from conftest import REPO
from refine_ref import rodrigues


def moved(R, t, c, delta):
    """The header's step: R' = Rd R, t' = Rd (t - c) + c + tau."""
    Rd = rodrigues(np.asarray(delta[:3], dtype=np.float64))
    return Rd @ R, Rd @ (t - c) + c + delta[3:]


def test_the_gradient_is_the_overlaps():
    """g against central differences of E = -O_AB along each of the six rigid directions, and H against the header's properties: symmetric
    by construction, positive semidefinite, the translation block w I."""
    for name, take in (("ref41", 4), ("ref2", 3), ("ref65", 2)):
        c = overlay_cases.case(name)
        for i in [i for i in range(c["n"]) if len(c["points"][i]) >= 3][:take]:  # (both kinds of row: the copies are the even ones)
            row = overlay_ref.Row(c["ref_xyz"], c["ref_radius"], c["points"][i], c["radii"][i] if c["radii"] is not None else np.float32(overlay_cases.NODE_RADIUS))
            R, t = c["R"][i], c["t"][i]
            H, g, cen = overlay_ref.normal_equations(row, R, t)
            O = overlay_ref.overlap(row, R, t)
            assert O > 0 and np.abs(g).max() > 0, (name, i)
            h = 1e-5
            for k in range(6):
                d = np.zeros(6)
                d[k] = h
                Rp, tp = moved(R, t, cen, d)
                Rm, tm = moved(R, t, cen, -d)
                fd = -(overlay_ref.overlap(row, Rp, tp) - overlay_ref.overlap(row, Rm, tm)) / (2 * h)
                assert abs(fd - g[k]) <= 1e-7 * max(np.abs(g).max(), O), (name, i, k, fd, g[k])
            assert np.linalg.eigvalsh(H).min() >= -1e-12 * np.trace(H), (name, i)
            assert H[3, 3] == H[4, 4] == H[5, 5] > 0 and H[3, 4] == H[3, 5] == H[4, 5] == 0 and H[0, 3] == H[1, 4] == H[2, 5] == 0


def test_a_moved_copy_of_the_6oim_ligand_comes_back():
    xyz, radius = overlay_cases.ligand_6oim()
    o_bb = shape_ref.self_overlap(xyz, radius)
    for shift in ([1.0, 0.0, 0.0], [-0.6, 0.7, 0.5]):
        trace = []
        out = overlay_ref.overlay_row(xyz, radius, xyz, radius, np.eye(3), np.array(shift), ftol=1e-12, max_iter=64, o_bb=o_bb, trace=trace)
        print(f"shift {shift}: Tanimoto {out['energy'][4]:.6f} -> {out['energy'][5]:.12f} in {out['count'][0]} evaluations, stop {out['count'][2]}")
        assert out["status"] == 0 and out["energy"][4] < 0.9 and abs(out["energy"][5] - 1.0) <= 1e-9
        assert abs(out["energy"][2] - o_bb) <= 1e-12 * o_bb and out["energy"][3] == o_bb  # (the shift rounds each coordinate: O_AA is O_BB to rounding)
        assert all(b > a for a, b in zip(trace, trace[1:])) and len(trace) == out["count"][1] + 1
        assert np.abs(shape_ref.pose(xyz, out["rotation"], out["translation"]) - xyz.astype(np.float64)).max() <= 1e-4


def test_o_ab_never_decreases_and_the_outputs_hang_together():
    for name in ("ref41", "ref2", "iter0", "iter1"):
        c = overlay_cases.case(name)
        for i in range(0, c["n"], 3):
            trace = []
            out = overlay_cases.reference_row(c, i, trace=trace)
            e, (iterations, accepted, stop, npts) = out["energy"], out["count"]
            assert all(b > a for a, b in zip(trace, trace[1:])) and e[1] >= e[0] and e[0] == trace[0] and e[1] == trace[-1]
            assert npts == len(c["points"][i]) and accepted <= iterations <= c["max_iter"] and stop in (0, 1, 2, 3)
            assert (stop == 0) == (npts == 0 or e[0] == 0)
            if accepted == 0:
                assert np.array_equal(out["rotation"], c["R"][i]) and np.array_equal(out["translation"], c["t"][i]) and e[6] == 0 and e[7] == 0
            assert 0 <= e[4] <= e[5] <= 1 + 1e-12
            R = out["rotation"]
            assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-13 + 10 * np.abs(c["R"][i].T @ c["R"][i] - np.eye(3)).max()


def test_rows_that_are_not_ok():
    xyz, radius = overlay_cases.ligand_6oim()
    pts = np.zeros((2, 3), np.float32)
    bad = np.eye(3)
    bad[0, 1] = np.nan
    for kw, status in ((dict(R=bad), 4), (dict(t=np.array([0, np.inf, 0])), 4), (dict(radii=np.array([1.0, 0.0], np.float32)), 4), (dict(radii=np.float32(np.nan)), 4),
                       (dict(points=np.zeros((257, 3), np.float32)), 1), (dict(status=1), 1)):
        args = dict(points=pts, radii=np.float32(1.0), R=np.eye(3), t=np.zeros(3))
        args.update(kw)
        out = overlay_ref.overlay_row(xyz, radius, o_bb=1.0, **args)
        assert out["status"] == status and np.isnan(out["rotation"]).all() and np.isnan(out["energy"]).all() and out["count"].tolist() == [0, 0, -1, 0]
    assert overlay_ref.starts_row(xyz, pts, 4)["status"] == 4 and overlay_ref.starts_row(xyz, pts, -1)["status"] == 4
    assert overlay_ref.starts_row(xyz, np.zeros((257, 3)), 0)["status"] == 1 and np.isnan(overlay_ref.starts_row(xyz, pts, 7)["frame"]).all()


def test_the_jacobi_frame():
    rng = np.random.default_rng(5)
    sets = [rng.normal(size=(n, 3)) * rng.uniform(0.5, 5, size=3) + rng.uniform(-20, 20, size=3) for n in (3, 4, 41, 64, 65, 256)]
    sets.append(overlay_cases.ligand_6oim()[0].astype(np.float64))
    sets.append(np.round(rng.normal(size=(30, 3))) * np.array([1.0, 1.0, 0.0]))  # planar, on a lattice: exact zeros among the sums
    for x in sets:
        c, ax, ev = overlay_ref.frame(x)
        d = x - x.mean(axis=0)
        C = d.T @ d
        E = ax.T  # the axes as columns
        D = E.T @ C @ E
        assert np.abs(D - np.diag(np.diag(D))).max() <= 1e-10 * np.trace(C), len(x)
        assert np.abs(E.T @ E - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(E) - 1.0) <= 1e-14
        assert ev[0] >= ev[1] >= ev[2] >= -1e-10 * np.trace(C) and np.allclose(ev, np.diag(D), rtol=1e-9, atol=1e-10 * np.trace(C)) and np.allclose(c, x.mean(axis=0))
    # the degenerate sets
    c, ax, ev = overlay_ref.frame(np.zeros((0, 3)))
    assert np.array_equal(c, np.zeros(3)) and np.array_equal(ax, np.eye(3)) and np.array_equal(ev, np.zeros(3))
    c, ax, ev = overlay_ref.frame(np.array([[1.0, -2.0, 3.0]]))
    assert np.array_equal(c, [1.0, -2.0, 3.0]) and np.array_equal(ax, np.eye(3)) and np.array_equal(ev, np.zeros(3))
    for x in (np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 2.0]]), np.outer(np.arange(5.0), [1.0, -1.0, 0.5]) + 3.0):  # two points; five on a line
        c, ax, ev = overlay_ref.frame(x)
        line = (x[-1] - x[0]) / np.linalg.norm(x[-1] - x[0])
        assert abs(abs(ax[0] @ line) - 1.0) <= 1e-14 and ev[0] > 0 and abs(ev[1]) <= 1e-14 * ev[0] and abs(ev[2]) <= 1e-14 * ev[0]
        assert np.abs(ax @ ax.T - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(ax) - 1.0) <= 1e-14


def test_one_of_the_four_starts_finds_a_turned_copy():
    xyz, radius = overlay_cases.ligand_6oim()
    o_bb = shape_ref.self_overlap(xyz, radius)
    rng = np.random.default_rng(11)
    for trial in range(3):
        Q, shift = shape_ref.random_rotations(rng, 1)[0], rng.uniform(-10, 10, size=3)
        copy = ((xyz.astype(np.float64) - xyz.mean(axis=0)) @ Q.T + shift).astype(np.float32)  # (rounded to float32: a copy to 1e-6 A)
        finals = []
        for s in range(4):
            st = overlay_ref.starts_row(xyz, copy, s)
            R = st["rotation"]
            assert st["status"] == 0 and np.abs(R.T @ R - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(R) - 1.0) <= 1e-14
            posed = shape_ref.pose(copy, R, st["translation"])
            assert np.abs(posed.mean(axis=0) - xyz.astype(np.float64).mean(axis=0)).max() <= 1e-12  # the centres coincide
            finals.append(overlay_ref.overlay_row(xyz, radius, copy, radius, R, st["translation"], ftol=1e-9, max_iter=64, o_bb=o_bb)["energy"][5])
        print(f"turned copy {trial}: final Tanimoto of the four starts {np.round(finals, 4).tolist()}")
        assert max(finals) > 0.999 and sorted(finals)[-2] < 0.95
    # the four starts differ by half turns about the row's axes
    a = [overlay_ref.starts_row(xyz, copy, s)["rotation"] for s in range(4)]
    for s in (1, 2, 3):
        half = a[0].T @ a[s]
        assert np.allclose(half @ half, np.eye(3), atol=1e-13) and abs(np.trace(half) + 1.0) <= 1e-13


def test_sensitivity_over_the_rows_of_the_gpu_tests():
    """S: over every seeded row the GPU tests use, the largest difference between the three variants of the restatement in posed point
    coordinates and in relative final O_AB. All three must agree in every integer on every row, and no row may stand within 1e-9 of a
    decision: the seeds of tests/overlay_cases.py are chosen so. The recorded figures (overlay_cases.S, one per case) are what the bars of
    the GPU tests are made of, so no case's measured one may exceed its record."""
    for name in overlay_cases.CASES:
        s_pts, s_o, agree, margin = overlay_cases.sensitivity(name)
        ref = overlay_cases.reference(name)
        stops = np.bincount(np.array([r["count"][2] for r in ref]) + 1, minlength=5).tolist()
        print(f"{name}: S points {s_pts:.3e} A, S overlap {s_o:.3e}, decision margin {margin:.3e}, stops (-1, 0, 1, 2, 3) {stops}, "
              f"mean evaluations {np.mean([r['count'][0] for r in ref]):.1f}")
        assert agree, name
        assert margin >= overlay_cases.MARGIN, (name, margin)
        assert max(s_pts, s_o) <= overlay_cases.S[name], (name, s_pts, s_o, overlay_cases.S[name])
        c = overlay_cases.case(name)
        counts = {len(p) for p in c["points"]}
        assert counts == set(overlay_cases.COUNTS) - ({1} if len(c["ref_xyz"]) == 1 else set()), name
        assert all(r["count"][2] == 0 for r, p in zip(ref, c["points"]) if len(p) == 0) and all(r["energy"][0] > 0 for r, p in zip(ref, c["points"]) if len(p)), name
        if len(c["ref_xyz"]) == 256:
            assert sum(len(p) == 256 for p in c["points"]) == overlay_cases.BIG_ROWS
    assert {len(overlay_cases.case(n)["ref_xyz"]) for n in overlay_cases.CASES} == set(overlay_cases.REF_SIZES)
    assert {overlay_cases.case(n)["max_iter"] for n in overlay_cases.CASES} == set(overlay_cases.MAX_ITERS)
    for name, reasons in (("ref41", {0, 1, 2}), ("iter0", {0, 2}), ("iter1", {0, 2})):
        assert reasons <= {int(r["count"][2]) for r in overlay_cases.reference(name)}, name


def test_the_flat_case_has_nothing_to_follow():
    c = overlay_cases.flat_case()
    for i in c["far"]:
        out = overlay_cases.reference_row(c, int(i))
        assert out["status"] == 0 and out["count"].tolist() == [0, 0, 0, len(c["points"][i])] and out["energy"][0] == 0 and out["energy"][5] == 0
        assert np.array_equal(out["rotation"], c["R"][i]) and np.array_equal(out["translation"], c["t"][i])
    for i in c["at_maximum"]:
        out = overlay_cases.reference_row(c, int(i))
        e = out["energy"]
        # (about 13 rejected trials: 1e-3 * 8^13 > 1e8; a trial that gains a last bit is taken and costs two more)
        assert out["status"] == 0 and e[0] == e[2] == e[3] and e[4] == 1.0 and e[1] >= e[0] and out["count"][2] == 3 and 13 <= out["count"][0] <= 32 and e[7] <= 1e-6


def test_header_binding_and_build_list():
    from pharmaconet_amd import _ffi, build

    text = (REPO / "include" / "pmx.h").read_text()
    assert int(re.search(r"#define PMX_SHAPE_JACOBI_SWEEPS (\d+)", text).group(1)) == overlay_ref.JACOBI_SWEEPS
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in (("pmx_shape_overlay", 19), ("pmx_shape_starts", 13)):
        decl = re.search(name + r"\s*\(([^;]*)\);", code).group(1)
        restype, argtypes = _ffi.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == n_args == decl.count(",") + 1, name
    assert _ffi.SIGNATURES["pmx_shape_overlay"][1][9:13] == [ctypes.c_uint32, ctypes.c_float, ctypes.c_double, ctypes.c_int]
    assert "pmx_shape_overlay.hip" in build.SOURCES and "pmx_shape.h" in build.DEPS
