"""CPU side of the pose-fit feature (`pmx_pose_fit`): the NumPy restatement of tests/pose_fit_ref.py against hand cases and against
tests/align_ref.py's pairs, the margins of the seeded cases the GPU tests run, and the C entry point: declared, bound and exported."""

import ctypes
import subprocess

import numpy as np
import pytest

import align_ref
import pose_fit_ref as pfr
from conftest import REPO, load_golden
from explain_ref import Tables
from test_align_cpu import explained_rows

MARGIN = 1e-9
EYE, ZERO = np.eye(3), np.zeros(3)


def hand_record(masks, positions):
    """The unpacked record of nodes with type masks `masks` at `positions` [n, 3] (one conformer)."""
    from ligand_fp_ref import make_record
    from pharmaconet_amd import PackedLibrary

    return PackedLibrary.from_records([make_record(masks, np.asarray(positions, dtype=np.float32).reshape(len(masks), 1, 3))]).unpack(0)


W7 = np.array([1.0, 4.0, 8.0, 8.0, 4.0, 4.0, 4.0], dtype=np.float32)


def test_a_node_on_a_centre_scores_its_weight_exactly():
    types, centers, sigmas = [1, 4], [[3.0, -2.0, 5.0], [10.0, 0.0, 0.0]], [1.25, 1.5]
    rec = hand_record([1 << 1, 1 << 4], [[3.0, -2.0, 5.0], [10.0, 0.0, 0.0]])
    r = pfr.fit_row(types, centers, sigmas, W7, rec, 0, EYE, ZERO)
    assert r["status"] == 0 and r["node_z2"].tolist() == [0.0, 0.0] and r["node_fit"].tolist() == [4.0, 4.0] and r["node_best"].tolist() == [4.0, 4.0]
    assert r["summary"].tolist() == [8.0, 8.0, 8.0, 8.0] and r["summary"][0] / r["summary"][1] == 1.0
    assert r["count"].tolist() == [2, 2, 2, 2] and r["node_target"].tolist() == [0, 1] and r["hotspot_node"].tolist() == [0, 1] and r["hotspot_z2"].tolist() == [0.0, 0.0]
    assert int(r["fingerprint"][0]) == 0b11 and not r["fingerprint"][1:].any()
    # under a motion that is exact in float64: a quarter turn about z and a shift
    turn = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    rec = hand_record([1 << 1], [[2.0, 1.0, 4.0]])  # R x + t = (-1, 2, 4) + (4, -4, 1)
    r = pfr.fit_row(types, centers, sigmas, W7, rec, 0, turn, [4.0, -4.0, 1.0])
    assert r["node_z2"].tolist() == [0.0] and r["summary"].tolist() == [4.0, 4.0, 4.0, 4.0]


def test_a_node_at_exactly_two_sigma_does_not_pass():
    """sigma = 1 and an offset of (2, 0, 0): d2 = 4 = 4 v exactly, and `<` is strict. One float32 step closer it passes."""
    inside = float(np.nextafter(np.float32(2), np.float32(0)))
    for x, passes in ((2.0, False), (inside, True)):
        r = pfr.fit_row([0], [[0.0, 0.0, 0.0]], [1.0], W7, hand_record([1], [[x, 0.0, 0.0]]), 0, EYE, ZERO)
        assert r["status"] == 0 and r["count"].tolist() == [1, 1, int(passes), int(passes)] and int(r["fingerprint"][0]) == int(passes)
        assert r["node_z2"][0] == x * x and r["node_fit"][0] == 1.0 * float(np.exp(-0.5 * (x * x))) and r["hotspot_node"].tolist() == [0]
    assert pfr.fit_row([0], [[0.0, 0.0, 0.0]], [1.0], W7, hand_record([1], [[2.0, 0.0, 0.0]]), 0, EYE, ZERO)["margin"] == 0.0


def test_far_away_nothing_is_occupied_and_the_fit_goes_to_zero():
    c = pfr.free_case(37, 1)
    i, conf = int(c["indices"][0]), int(c["conformers"][0])
    rec = c["lib"].unpack(i)
    near = pfr.fit_row(c["node_type"], c["centers"], c["sigmas"], c["w7"], rec, conf, c["rotation"][0], c["translation"][0])
    far = pfr.fit_row(c["node_type"], c["centers"], c["sigmas"], c["w7"], rec, conf, c["rotation"][0], c["translation"][0] + 1000.0)
    assert near["summary"][0] > 0 and far["summary"][0] == 0.0 and far["summary"][2] == 0.0 and far["summary"][1] == near["summary"][1] > 0
    assert not far["fingerprint"].any() and far["count"].tolist() == [near["count"][0], near["count"][1], 0, 0]
    # a weight of 0 takes the type out, a sigma that is no positive number its model node
    w0 = c["w7"].copy()
    w0[int(c["node_type"][near["node_target"][0]])] = 0.0
    assert all(c["node_type"][m] != c["node_type"][near["node_target"][0]] for _, m, _, _ in pfr.fit_row(c["node_type"], c["centers"], c["sigmas"], w0, rec, conf, EYE, ZERO)["pairs"])
    for bad in (0.0, np.nan, -1.0, np.inf):
        s = c["sigmas"].copy()
        s[3] = bad
        got = pfr.fit_row(c["node_type"], c["centers"], s, c["w7"], rec, conf, c["rotation"][0], c["translation"][0])
        assert all(m != 3 for _, m, _, _ in got["pairs"]) and np.isinf(got["hotspot_z2"][3]) and got["hotspot_node"][3] == -1
        assert [q for q in near["pairs"] if q[1] != 3] == got["pairs"]
    # statuses
    assert pfr.fit_row(c["node_type"], c["centers"], c["sigmas"], c["w7"], None, 0, EYE, ZERO)["status"] == 1
    for cc, R in ((-1, EYE), (1, EYE), (0, np.full((3, 3), np.nan))):
        bad = pfr.fit_row(c["node_type"], c["centers"], c["sigmas"], c["w7"], rec, cc, R, ZERO)
        assert bad["status"] == 4 and np.isnan(bad["summary"]).all() and not bad["count"].any() and np.isnan(bad["hotspot_z2"]).all() and (bad["node_target"] == -1).all()


def test_key_mode_pairs_are_align_refs_and_a_subset_of_the_free_ones():
    from pharmaconet_amd.constants import weights_vector

    model, lib, weights, _ = load_golden("set_6oim_c8")
    w7 = weights_vector(weights)
    types, Y, S = np.asarray(model.flat.node_type), model.node_centers, model.node_radii
    assert S.shape == (model.num_nodes,) and (S > 0.9).all() and (S < 1.7).all() and S.dtype == np.float64
    seen = 0
    for i, c, lv, key in list(explained_rows("set_6oim_c8"))[:24]:
        rec = lib.unpack(i)
        al = align_ref.align(model, rec, w7, lv, key, c, Tables(model, rec, w7), "svd", Y)
        pairs = pfr.key_pairs(model, rec, w7, lv, key, c)
        assert al["valid"] and pairs is not None
        k = pfr.fit_row(types, Y, S, w7, rec, c, al["R"], al["t"], pairs)
        f = pfr.fit_row(types, Y, S, w7, rec, c, al["R"], al["t"])
        assert k["status"] == 0 and (int(k["count"][0]), int(k["count"][1])) == (al["n_nodes"], al["n_pairs"])
        assert {(u, m) for u, m, _, _ in k["pairs"]} <= {(u, m) for u, m, _, _ in f["pairs"]}
        assert dict(((u, m), z) for u, m, z, _ in k["pairs"]).items() <= dict(((u, m), z) for u, m, z, _ in f["pairs"]).items()
        assert 0 <= k["summary"][0] <= k["summary"][1] and k["count"][3] <= k["count"][1] and k["count"][2] <= k["count"][0]
        seen += al["n_pairs"] > 0
        # a match that is no candidate of its level
        if len(lv) and seen == 1:
            from explain_ref import candidates

            wrong = next(a for a in range(model.flat.num_clusters) if a not in candidates(model, rec, int(lv[0])))
            assert pfr.key_pairs(model, rec, w7, lv, [wrong] + list(key[1:]), c) is None
    assert seen >= 8


@pytest.mark.parametrize("nm,stride", pfr.FREE_CASES)
def test_seeded_cases_stand_clear_of_every_threshold(nm, stride):
    """What lets the GPU tests ask for equal integers: no pair of a seeded case within 1e-9 of the 2-sigma threshold, no node and no hotspot
    whose two best z2 differ by less than that. About half the nodes with a pair are within 2 sigma of a hotspot."""
    c = pfr.free_case(nm, stride)
    margin = min(r["margin"] for r in c["ref"])
    nodes = sum(int(r["count"][0]) for r in c["ref"])
    placed = sum(int(np.count_nonzero((r["node_z2"] >= 0) & (r["node_z2"] < 4.0))) for r in c["ref"])
    print(f"{nm} model nodes, stride {stride}: margin {margin:.3e}, {placed} of {nodes} nodes within 2 sigma of a hotspot, {sum(int(r['count'][1]) for r in c['ref'])} pairs")
    assert margin >= MARGIN
    assert all(r["status"] == 0 for r in c["ref"]) and len(c["ref"]) == pfr.ROWS and len(c["node_type"]) == nm == c["model"].flat.num_nodes
    assert sorted(set(c["counts"]))[:2] == [1, 2] and {63, 64} <= set(c["counts"]) and int(c["lib"].headers()[:, 1].max()) == stride
    assert nodes > 0 and 0.3 * nodes <= placed <= 0.85 * nodes


def test_header_declares_and_ffi_binds_pmx_pose_fit():
    from pharmaconet_amd import _ffi
    from pharmaconet_amd.build import DEPS, SOURCES

    text = (REPO / "include" / "pmx.h").read_text()
    assert "int pmx_pose_fit(const pmx_model *model, const pmx_library *lib, const float weights[PMX_NUM_TYPES]," in text
    assert "const double *node_sigma_dev" in text and "uint64_t *occupied_fp_dev" in text
    restype, argtypes = _ffi.SIGNATURES["pmx_pose_fit"]
    assert restype is ctypes.c_int and len(argtypes) == 22 and argtypes[10] is ctypes.c_uint32
    assert "pmx_pose_fit.hip" in SOURCES and "pmx_rows_front.h" in DEPS


def test_library_exports_pmx_pose_fit_and_checks_its_arguments():
    import __graft_entry__ as entry

    entry.build()
    from pharmaconet_amd import _ffi

    syms = subprocess.run(["nm", "-D", "--defined-only", str(_ffi.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert " T pmx_pose_fit\n" in syms
    lib = _ffi.load()
    assert lib.pmx_pose_fit(None, None, None, *([None] * 7), 1, *([None] * 10), None) == 1 and b"null" in lib.pmx_last_error()
