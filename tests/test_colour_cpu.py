"""`pmx_pose_colour` and `pmx_combo_overlay` without a GPU: the NumPy restatements (tests/colour_ref.py, tests/combo_ref.py) against what
the header promises - the reference on itself has a colour Tanimoto of exactly 1, the gradient is F's, H is positive semidefinite, F never
decreases - the sensitivity figure S over exactly the seeded rows of the GPU tests (tests/combo_cases.py), from which their bars follow,
and the Python layer that needs no device: `ColourFeatures` and `ReferenceLigand.from_library`."""

import ctypes
import re

import numpy as np
import pytest

import colour_ref
import combo_cases
import combo_ref
import overlay_ref
import shape_ref
from conftest import REPO, load_golden
from refine_ref import rodrigues


def moved(R, t, c, delta):
    """The header's step: R' = Rd R, t' = Rd (t - c) + c + tau."""
    Rd = rodrigues(np.asarray(delta[:3], dtype=np.float64))
    return Rd @ R, Rd @ (t - c) + c + delta[3:]


def rows_of(c, i):
    pts, rad = combo_cases.shape_points(c, i)
    return (overlay_ref.Row(c["ref_xyz"], c["ref_radius"], pts, rad),
            combo_ref.TypedRow(c["feat_xyz"], c["feat_mask"], c["weights"], combo_cases.COLOUR_RADIUS, c["nodes"][i], c["masks"][i]))


def test_the_reference_on_itself_has_colour_tanimoto_one():
    for name in ("f1", "f2_nodes", "f63", "f64"):
        c = combo_cases.case(name)
        out = colour_ref.colour_row(c["feat_xyz"], c["feat_mask"], c["weights"], combo_cases.COLOUR_RADIUS, c["feat_xyz"], c["feat_mask"], np.eye(3), np.zeros(3), c_bb=c["c_bb"])
        s = out["summary"]
        assert out["status"] == 0 and s[0] == s[1] == s[2] == c["c_bb"] > 0 and s[3] == 1.0 and s[4] == 1.0 and s[5] == 1.0, name
        typed = np.array([combo_cases.colour_ref.weight_table(c["weights"])[int(m)] != 0 for m in c["feat_mask"]])
        assert np.array_equal(out["node_feature"][: len(typed)] >= 0, typed) and (out["node_near"][: len(typed)][typed] == 0).all() and s[6] == 0.0, name
        assert out["counts"].tolist() == [len(typed), int(typed.sum()), int(typed.sum()), len(typed)], name
        assert abs(out["type_overlap"].sum() - s[0]) <= 1e-13 * s[0], name  # (the parts add up to C_AB up to rounding)


def test_exact_consequences_of_the_pair_term():
    w = np.array(combo_cases.DEFAULT, np.float32)
    one = colour_ref.colour_row([[1.0, 2.0, 3.0]], [0b1100], w, 1.0, [[1.0, 2.0, 3.0]], [0b0101], np.eye(3), np.zeros(3))
    q = shape_ref.PI / (colour_ref.alpha_c(1.0) + colour_ref.alpha_c(1.0))
    assert one["summary"][0] == 8.0 * (8.0 * (q * np.sqrt(q))) and one["type_overlap"].tolist() == [0, 0, one["summary"][0], 0, 0, 0, 0]  # the shared type: Cation, weight 8
    far = colour_ref.colour_row([[1.0, 2.0, 3.0]], [0b1100], w, 1.0, [[1.0, 2.0, 3.0]], [0b0101], np.eye(3), np.array([200.0, 0, 0]))
    assert far["summary"][0] == 0.0 and far["summary"][3] == 0.0 and far["node_feature"][0] == 0 and far["counts"].tolist() == [1, 0, 0, 1]
    none = colour_ref.colour_row([[1.0, 2.0, 3.0]], [0b0001], combo_cases.NO_HYDROPHOBIC, 1.0, [[1.0, 2.0, 3.0]], [0b0001], np.eye(3), np.zeros(3))
    assert none["summary"][0] == 0.0 and none["summary"][3] == 0.0 and none["node_feature"][0] == -1 and np.isnan(none["summary"][6]) and none["fp"] == 0
    both = colour_ref.colour_row([[0.0, 0.0, 0.0]], [0b0110], w, 1.0, [[0.0, 0.0, 0.0]], [0b0110], np.eye(3), np.zeros(3))
    assert both["summary"][0] == (4.0 + 8.0) * (8.0 * (q * np.sqrt(q)))  # two shared types: the weights add, ascending


def test_rows_that_are_not_ok():
    w = combo_cases.DEFAULT
    bad = np.eye(3)
    bad[1, 2] = np.nan
    pts, mk = np.zeros((2, 3), np.float32), [1, 2]
    for kw, status in ((dict(R=bad), 4), (dict(t=np.array([0, np.inf, 0])), 4), (dict(masks=[1, 128]), 4), (dict(points=np.zeros((65, 3), np.float32), masks=[1] * 65), 1),
                       (dict(status=1), 1)):
        args = dict(points=pts, masks=mk, R=np.eye(3), t=np.zeros(3))
        args.update(kw)
        out = colour_ref.colour_row([[0.0, 0.0, 0.0]], [1], w, 1.0, c_bb=1.0, **args)
        assert out["status"] == status and np.isnan(out["summary"]).all() and np.isnan(out["type_overlap"]).all() and out["counts"].tolist() == [0, 0, 0, 0] and out["fp"] == 0
        assert np.isnan(out["node_near"]).all() and (out["node_feature"] == -1).all() and (out["feat_node"] == -1).all()
    for kw, status in ((dict(R=bad), 4), (dict(radii=np.float32(0.0)), 4), (dict(masks=[1, 200]), 4), (dict(points=np.zeros((257, 3), np.float32)), 1), (dict(status=4), 4)):
        args = dict(points=pts, radii=np.float32(1.0), nodes=pts, masks=mk, R=np.eye(3), t=np.zeros(3))
        args.update(kw)
        out = combo_ref.combo_row([[0.0, 0.0, 0.0]], [1.7], [[0.0, 0.0, 0.0]], [1], w, 1.0, colour_weight=1.0, o_bb=1.0, c_bb=1.0, **args)
        assert out["status"] == status and np.isnan(out["rotation"]).all() and np.isnan(out["energy"]).all() and out["count"].tolist() == [0, 0, -1, 0, 0, 0]


def test_the_gradient_is_f_s_and_h_is_positive_semidefinite():
    """g against central differences of E = -F along each of the six rigid directions, H against the header's properties."""
    for name, take in (("f63", 4), ("f2_nodes", 3), ("big", 2), ("f64", 2)):
        c = combo_cases.case(name)
        cw = c["cw"]
        assert cw > 0
        for i in [i for i in range(c["n"]) if len(combo_cases.shape_points(c, i)[0]) >= 3 and len(c["nodes"][i]) >= 3][:take]:
            row, trow = rows_of(c, i)
            R, t = c["R"][i], c["t"][i]
            H, g, cen = combo_ref.normal_equations(row, trow, cw, R, t)
            ev = combo_ref.evaluate(row, trow, cw, R, t)
            F = ev["F"]
            assert F > 0 and ev["cab"] > 0 and np.abs(g).max() > 0, (name, i)
            h = 1e-5
            for k in range(6):
                d = np.zeros(6)
                d[k] = h
                Rp, tp = moved(R, t, cen, d)
                Rm, tm = moved(R, t, cen, -d)
                fd = -(combo_ref.objective(row, trow, cw, Rp, tp) - combo_ref.objective(row, trow, cw, Rm, tm)) / (2 * h)
                assert abs(fd - g[k]) <= 1e-7 * max(np.abs(g).max(), F), (name, i, k, fd, g[k])
            assert np.linalg.eigvalsh(H).min() >= -1e-12 * np.trace(H), (name, i)
            assert H[3, 3] == H[4, 4] == H[5, 5] > 0 and H[3, 4] == H[3, 5] == H[4, 5] == 0 and H[0, 3] == H[1, 4] == H[2, 5] == 0


def test_f_never_decreases_and_the_outputs_hang_together():
    for name in ("f63", "f2_nodes", "cw0", "iter0", "iter1"):
        c = combo_cases.case(name)
        for i in range(0, c["n"], 3):
            trace = []
            out = combo_cases.reference_row(c, i, trace=trace)
            e, (iterations, accepted, stop, npts, nn, f) = out["energy"], out["count"]
            assert all(b > a for a, b in zip(trace, trace[1:])) and out["F"] == (trace[0], trace[-1]) and len(trace) == accepted + 1
            assert npts == len(combo_cases.shape_points(c, i)[0]) and nn == len(c["nodes"][i]) and f == len(c["feat_mask"])
            assert accepted <= iterations <= c["max_iter"] and stop in (0, 1, 2, 3) and (stop == 0) == (out["F"][0] == 0)
            if accepted == 0:
                assert np.array_equal(out["rotation"], c["R"][i]) and np.array_equal(out["translation"], c["t"][i]) and e[14] == 0 and e[15] == 0 and e[0] == e[1] and e[6] == e[7]
            assert 0 <= e[4] <= 1 + 1e-12 and 0 <= e[5] <= 1 + 1e-12 and 0 <= e[10] <= 1 + 1e-12 and 0 <= e[11] <= 1 + 1e-12
            assert e[12] == e[4] + e[10] and e[13] == e[5] + e[11] and e[3] == c["o_bb"] and e[9] == c["c_bb"]
            if c["cw"] == 0:  # the shape overlay's row, bit for bit
                pts, rad = combo_cases.shape_points(c, i)
                sh = overlay_ref.overlay_row(c["ref_xyz"], c["ref_radius"], pts, rad, c["R"][i], c["t"][i], ftol=combo_cases.FTOL, max_iter=c["max_iter"], o_bb=c["o_bb"])
                assert np.array_equal(sh["rotation"], out["rotation"]) and np.array_equal(sh["translation"], out["translation"]) and np.array_equal(sh["count"], out["count"][:4])
                assert np.array_equal(sh["energy"][:6], e[:6]) and np.array_equal(sh["energy"][6:], e[14:])


def test_sensitivity_over_the_rows_of_the_gpu_tests():
    """S: over every seeded row the GPU tests use, the largest difference between the three variants of the restatement in posed point
    coordinates and in relative final F. All three must agree in every integer on every row, and no row may stand within 1e-9 of a
    decision: the seeds of tests/combo_cases.py are chosen so. The recorded figures (combo_cases.S, one per case) are what the bars of the
    GPU tests are made of, so no case's measured one may exceed its record."""
    seen_nodes, seen_points, seen_masks = set(), set(), set()
    for name in combo_cases.CASES:
        s_pts, s_f, agree, margin = combo_cases.sensitivity(name)
        ref = combo_cases.reference(name)
        c = combo_cases.case(name)
        stops = np.bincount(np.array([r["count"][2] for r in ref]) + 1, minlength=5).tolist()
        colour_margin = min(r["margin"] for r in combo_cases.colour_reference(name))
        print(f"{name}: S points {s_pts:.3e} A, S F {s_f:.3e}, decision margin {margin:.3e}, colour margin {colour_margin:.3e}, stops (-1, 0, 1, 2, 3) {stops}, "
              f"colour_weight {c['cw']:.4f}, mean evaluations {np.mean([r['count'][0] for r in ref]):.1f}")
        assert agree, name
        assert margin >= combo_cases.MARGIN and colour_margin >= combo_cases.MARGIN, (name, margin, colour_margin)
        assert max(s_pts, s_f) <= combo_cases.S[name], (name, s_pts, s_f, combo_cases.S[name])
        assert all(r["status"] == 0 for r in ref), name
        nodes = {len(x) for x in c["nodes"]}
        assert set(combo_cases.NODE_COUNTS) <= nodes, name
        seen_nodes |= nodes
        if c["points"] is not None:
            points = {len(p) for p in c["points"]}
            assert set(combo_cases.POINT_COUNTS) <= points, name
            seen_points |= points
        if len(c["ref_xyz"]) == 256:
            assert sum(len(p) == 256 for p in c["points"]) == combo_cases.BIG_ROWS
        for mk in c["masks"] + [c["feat_mask"]]:
            seen_masks |= {"zero" if m == 0 else "single" if bin(int(m)).count("1") == 1 else "multi" for m in mk}
    assert {len(combo_cases.case(n)["feat_mask"]) for n in combo_cases.CASES} >= set(combo_cases.FEATURE_SIZES)
    assert {combo_cases.case(n)["max_iter"] for n in combo_cases.CASES} == set(combo_cases.MAX_ITERS)
    assert seen_masks == {"zero", "single", "multi"} and any(0.0 in combo_cases.CASES[n][3] for n in combo_cases.CASES)
    cws = {combo_cases.CASES[n][4] for n in combo_cases.CASES}
    assert cws == {0.0, 1.0, None}  # (None: balanced)
    for name, reasons in (("f63", {1, 2}), ("iter0", {2}), ("iter1", {0, 2}), ("f2_nodes", {0, 1, 2})):
        assert reasons <= {int(r["count"][2]) for r in combo_cases.reference(name)}, name


# ---------------------------------------------------------------------------------------------------------------- the Python layer
def test_colour_features_from_arrays_csv_and_library(tmp_path):
    from pharmaconet_amd.constants import DEFAULT_WEIGHTS, TYPE_NAMES
    from pharmaconet_amd.shape import ColourFeatures, ReferenceLigand, type_masks

    xyz = np.array([[1.5, -2.25, 3.0], [0.1, 0.2, 0.3], [7.0, 8.0, 9.0]], np.float32)
    a = ColourFeatures.from_arrays(xyz, ["Anion", "Aromatic", "HBond_donor"])
    assert a.typemask.tolist() == [8, 2, 16] and a.weights == DEFAULT_WEIGHTS and a.radius == 1.0 and len(a) == 3 and a.types(0) == ["Anion"]
    assert ColourFeatures.from_arrays(xyz, [3, 1, 4]).typemask.tolist() == [8, 2, 16]
    assert ColourFeatures.from_arrays(xyz, np.array([8, 6, 0], np.uint8)).typemask.tolist() == [8, 6, 0]
    assert ColourFeatures.from_arrays(xyz, [3, 1, 4], weights={"Anion": 0.0}).weights_array().tolist() == [1, 4, 8, 0, 4, 4, 4]
    assert type_masks(list(TYPE_NAMES)).tolist() == [1, 2, 4, 8, 16, 32, 64]
    path = tmp_path / "ref.csv"
    a.to_csv(path)
    b = ColourFeatures.from_csv(path)
    assert np.array_equal(b.xyz, a.xyz) and np.array_equal(b.typemask, a.typemask)
    several = ColourFeatures.from_arrays(xyz, np.array([0b0110, 0, 0b1000001], np.uint8))
    several.to_csv(path)
    assert path.read_text().splitlines()[1].startswith("Aromatic|Cation,1.5,-2.25,3.0") and len(path.read_text().splitlines()) == 3  # (the feature without a type is left out)
    back = ColourFeatures.from_csv(path)
    assert back.typemask.tolist() == [0b0110, 0b1000001] and np.array_equal(back.xyz, xyz[[0, 2]]) and type_masks(["Anion|Cation"]).tolist() == [12]
    path.write_text("# a known binder\ntype,x,y,z\nAnion, 1.5, -2.25, 3\n\nCarboxylate,0,0,0\n")
    with pytest.raises(ValueError, match="Carboxylate"):
        ColourFeatures.from_csv(path)
    for bad in (dict(xyz=xyz, types=["Anion"]), dict(xyz=np.zeros((0, 3)), types=[]), dict(xyz=np.zeros((65, 3)), types=[0] * 65), dict(xyz=xyz, types=[0, 1, 7]),
                dict(xyz=xyz * np.nan, types=[0, 1, 2]), dict(xyz=xyz, types=[0, 1, 2], radius=0.0), dict(xyz=xyz, types=[0, 1, 2], weights={"Anion": -1.0}),
                dict(xyz=xyz, types=[0, 1, 2], weights={"Anion": float("nan")}), dict(xyz=xyz, types=np.array([1, 2, 128], np.uint8)), dict(xyz=xyz, types=["Anion", "anion", "Anion"])):
        with pytest.raises(ValueError):
            ColourFeatures.from_arrays(**bad)

    _, lib, _, _ = load_golden("set_6oim_c8")
    rec = lib.unpack(3)
    got = ColourFeatures.from_library(lib, 3, conformer=2)
    assert np.array_equal(got.xyz, rec["xyz"][:, :, 2]) and np.array_equal(got.typemask, rec["typemask"])
    R, t = shape_ref.random_rotations(np.random.default_rng(1), 1)[0], np.array([1.0, -2.0, 0.5])
    posed = ColourFeatures.from_library(lib, 3, conformer=2, rotation=R, translation=t)
    assert np.array_equal(posed.xyz, shape_ref.pose(rec["xyz"][:, :, 2], R, t).astype(np.float32)) and np.array_equal(posed.typemask, rec["typemask"])
    with pytest.raises(ValueError):
        ColourFeatures.from_library(lib, 3, conformer=rec["n_conf"])
    both = ReferenceLigand.from_library(lib, 3, 2, node_radius=1.25)
    assert np.array_equal(both.xyz, got.xyz) and (both.radius == np.float32(1.25)).all() and np.array_equal(both.colour.xyz, got.xyz)
    assert ReferenceLigand.from_arrays(xyz, [1.0, 1.0, 1.0]).colour is None


def test_the_atoms_of_a_library_reference(tmp_path):
    from pharmaconet_amd.atoms import PackedAtoms
    from pharmaconet_amd.pocket import atomic_number_radii
    from pharmaconet_amd.shape import ReferenceLigand

    _, lib, _, _ = load_golden("set_6oim_c8")
    rng = np.random.default_rng(2)
    heads = lib.headers()
    elements = [rng.choice([1, 6, 7, 8, 16], size=12) for _ in range(len(lib))]
    positions = [rng.normal(size=(12, int(heads[i, 1]), 3)).astype(np.float32) for i in range(len(lib))]
    store = PackedAtoms.from_arrays(elements, positions)
    ref = ReferenceLigand.from_library(lib, 1, 0, atoms=store)
    heavy = elements[1] > 1
    assert np.array_equal(ref.xyz, positions[1][heavy, 0]) and np.array_equal(ref.radius, atomic_number_radii(elements[1][heavy])) and len(ref.colour) == heads[1, 0]


def test_header_binding_and_build_list():
    from pharmaconet_amd import _ffi, build

    text = (REPO / "include" / "pmx.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in (("pmx_colour_ref_create", 7), ("pmx_colour_ref_self", 2), ("pmx_colour_ref_destroy", 1), ("pmx_pose_colour", 22), ("pmx_combo_overlay", 21)):
        decl = re.search(name + r"\s*\(([^;]*)\);", code).group(1)
        restype, argtypes = _ffi.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == n_args == decl.count(",") + 1, name
    assert _ffi.SIGNATURES["pmx_combo_overlay"][1][10:15] == [ctypes.c_uint32, ctypes.c_float, ctypes.c_double, ctypes.c_double, ctypes.c_int]
    assert _ffi.SIGNATURES["pmx_pose_colour"][1][9:11] == [ctypes.c_uint32, ctypes.c_float]
    assert "pmx_colour.hip" in build.SOURCES and "pmx_shape.h" in build.DEPS and "pmx_lm.h" in build.DEPS
    for doc in ("README.md", "DESIGN.md"):
        assert "pmx_colour.hip" in (REPO / doc).read_text(), doc
