"""CPU side of the pose search (`pmx_pose_search`): the C entry point - declared, bound, exported and checking its arguments -, the selection
rule of tests/pose_search_ref.py on hand-made arrays, and the NumPy chain (tests/align_ref.py, tests/clash_ref.py, the rule) on the 13
ligands of tests/golden/modes_set_6oim_c8.npz: how many hits get a passing pose from one pose, from all conformers, and from all conformers
under four binding modes - and how far every decision of that chain stands from a threshold, which is what entitles the GPU test to ask
for the same choices."""

import ctypes
import subprocess
from functools import lru_cache

import numpy as np
import pytest

import pose_search_ref as psr
from conftest import GOLDEN, REPO, load_golden

MARGIN = 1e-9  # the bar of tests/test_gpu_clash.py: no pair of a candidate row within this of a threshold
GAP = 1e-9  # two overlaps are the same bits, or this far apart (relative)


# ---------------------------------------------------------------------------------------------------------------- the entry point
def test_header_declares_pmx_pose_search():
    text = (REPO / "include" / "pmx.h").read_text()
    assert "int pmx_pose_search(const pmx_model *model, const pmx_library *lib, const float weights[PMX_NUM_TYPES], const double *node_center_dev," in text
    assert "uint64_t pmx_pose_search_work_bytes(uint32_t n, int n_modes, int conf_stride);" in text
    assert "then the lowest c, then the lowest m" in text  # (the definition is stated there)


def test_ffi_binds_pmx_pose_search():
    from pharmaconet_amd import _ffi

    restype, argtypes = _ffi.SIGNATURES["pmx_pose_search"]
    assert restype is ctypes.c_int and len(argtypes) == 37 and argtypes[6] is ctypes.c_uint32 and argtypes[17] is ctypes.c_double
    assert _ffi.SIGNATURES["pmx_pose_search_work_bytes"][0] is ctypes.c_uint64
    assert _ffi.EXPLAIN_MAX == 65536 and _ffi.MAX_CONFORMERS == 64 and _ffi.MAX_MODES == 8


def test_library_exports_pmx_pose_search_and_checks_its_arguments():
    import __graft_entry__ as entry

    entry.build()
    from pharmaconet_amd import _ffi

    syms = subprocess.run(["nm", "-D", "--defined-only", str(_ffi.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert " T pmx_pose_search\n" in syms and " T pmx_pose_search_work_bytes\n" in syms
    lib = _ffi.load()
    fake = ctypes.create_string_buffer(256)  # (stands for a model, a library and a pocket: no call below gets as far as reading one)
    addr = ctypes.addressof(fake)
    w = (ctypes.c_float * _ffi.NUM_TYPES)(*([1.0] * _ffi.NUM_TYPES))

    def call(n=1, n_modes=4, conf_stride=8, radius=1.0, tolerance=0.5, contact=4.5, max_clashing=0, min_fitted=1, min_fraction=0.0, handles=(addr, addr, w, addr), ptr=None):
        model, library, weights, pocket = handles
        rc = lib.pmx_pose_search(model, library, weights, ptr, pocket, ptr, n, ptr, ptr, ptr, n_modes, conf_stride, radius, tolerance, contact, max_clashing, min_fitted,
                                 min_fraction, *([ptr] * 16), ptr, 0, None)
        return rc, lib.pmx_last_error()

    for handles in ((None, addr, w, addr), (addr, None, w, addr), (addr, addr, None, addr), (addr, addr, w, None)):
        rc, msg = call(handles=handles)
        assert rc == 1 and b"null" in msg
    assert call(n=0)[0] == 0  # n = 0 succeeds
    for bad in (dict(n_modes=0), dict(n_modes=9), dict(conf_stride=0), dict(conf_stride=65)):
        rc, msg = call(n=0, **bad)
        assert rc == 1 and (b"n_modes" in msg or b"conf_stride" in msg), bad
    for bad in (dict(min_fraction=float("nan")), dict(min_fraction=1.5), dict(min_fraction=-0.1)):
        rc, msg = call(n=0, **bad)
        assert rc == 1 and b"min_fraction" in msg, bad
    for bad in (dict(max_clashing=-1), dict(min_fitted=0), dict(radius=float("inf")), dict(tolerance=float("nan")), dict(contact=float("nan"))):
        assert call(n=0, **bad)[0] == 1, bad
    # 65536 slots pass the count (the next check, of the pointers, stops the call), 65537 do not
    rc, msg = call(n=2048, n_modes=4, conf_stride=8)
    assert rc == 1 and b"null" in msg and b"65536" not in msg
    rc, msg = call(n=65537, n_modes=1, conf_stride=1)
    assert rc == 1 and b"65537" in msg and b"65536" in msg
    rc, msg = call(n=8193, n_modes=8, conf_stride=1)
    assert rc == 1 and b"65544" in msg
    # the size query
    size = lib.pmx_pose_search_work_bytes
    assert size(0, 1, 1) > 0 and size(1, 1, 1) > 0
    assert size(1, 1, 1) <= size(2, 1, 1) <= size(2, 2, 1) <= size(2, 2, 2) <= size(128, 8, 64)
    assert size(16, 4, 8) < size(32, 4, 8) and size(16, 4, 8) < size(16, 8, 8) and size(16, 4, 8) < size(16, 4, 16)
    assert size(128, 8, 64) >= 65536 * (9 + 3 + 8 + 64 + 4 + 64) * 8  # (at least the float64 outputs of the two calls on every slot)
    assert size(1, 0, 1) == 0 and size(1, 9, 1) == 0 and size(1, 1, 65) == 0 and size(129, 8, 64) == 0


# ---------------------------------------------------------------------------------------------------------------- the rule
def rule(value, clashing=None, overlap=None, align_ok=None, fitted=None, clash_ok=None, **kw):
    value = np.asarray(value, dtype=np.float64)
    full = lambda a, fill, dt: np.full(value.shape, fill, dt) if a is None else np.asarray(a, dtype=dt)  # noqa: E731
    return psr.choose(value, full(align_ok, True, bool), full(fitted, 3, np.int64), full(clash_ok, True, bool), full(clashing, 0, np.int64), full(overlap, 0.0, np.float64), **kw)


def test_rule_ties_on_value_go_to_the_lower_conformer_then_the_lower_mode():
    #        c = 0    1    2
    v = [[3.0, 5.0, 5.0],  # m = 0
         [5.0, 2.0, 5.0]]  # m = 1
    r = rule(v)
    assert (r["conformer"], r["mode"], r["passes"]) == (0, 1, True) and r["value"] == 5.0 and r["fraction"] == 1.0  # the lower conformer, though its mode is higher
    assert (r["n_candidates"], r["n_passing"], r["n_dropped"]) == (6, 6, 0)
    r = rule([[3.0, 5.0, 2.0], [1.0, 5.0, 5.0]])
    assert (r["conformer"], r["mode"]) == (1, 0)  # the same conformer twice: the lower mode
    clashing = [[0, 1, 1], [1, 0, 0]]
    r = rule(v, clashing=clashing, overlap=np.array(clashing) * 0.5)
    assert (r["conformer"], r["mode"], r["value"], r["n_passing"]) == (2, 1, 5.0, 3)  # only passing slots compete: (0, 1) clashes
    assert rule(v, clashing=clashing, max_clashing=1)["conformer"] == 0


def test_rule_without_a_passing_slot_takes_the_smallest_overlap():
    v = [[4.0, 9.0, 6.0], [3.0, 8.0, 7.0]]
    ones = np.ones((2, 3), np.int64)
    r = rule(v, clashing=ones, overlap=[[2.0, 3.0, 0.25], [5.0, 0.5, 0.75]])
    assert (r["conformer"], r["mode"], r["passes"], r["value"]) == (2, 0, False, 6.0) and r["fraction"] == 6.0 / 9.0
    assert (r["n_candidates"], r["n_passing"]) == (6, 0)
    # bit-equal overlaps: the larger value, then the lower conformer, then the lower mode
    r = rule(v, clashing=ones, overlap=[[0.25, 3.0, 0.25], [0.25, 0.25, 0.75]])
    assert (r["conformer"], r["mode"], r["value"]) == (1, 1, 8.0)
    r = rule([[4.0, 4.0, 4.0], [4.0, 4.0, 4.0]], clashing=ones, overlap=[[0.5, 0.25, 0.25], [0.25, 0.25, 0.75]])
    assert (r["conformer"], r["mode"]) == (0, 1)
    r = rule([[4.0, 4.0, 4.0], [4.0, 4.0, 4.0]], clashing=ones, overlap=[[0.5, 0.25, 0.25], [0.5, 0.25, 0.75]])
    assert (r["conformer"], r["mode"]) == (1, 0)
    # one ulp apart is apart
    r = rule([[4.0, 9.0]], clashing=[[1, 1]], overlap=[[0.25, np.nextafter(0.25, 1.0)]])
    assert r["conformer"] == 0
    # a passing slot beats any overlap, whatever it scores
    r = rule(v, clashing=[[1, 1, 1], [0, 1, 1]], overlap=[[2.0, 3.0, 0.25], [0.0, 0.5, 0.75]])
    assert (r["conformer"], r["mode"], r["passes"], r["value"]) == (0, 1, True, 3.0)


def test_rule_min_fraction_drops_and_counts():
    v = [[10.0, 4.0, 5.0], [4.99, 0.0, 5.0]]
    clashing = [[1, 0, 1], [0, 0, 1]]
    ov = np.array(clashing, np.float64)
    r = rule(v, clashing=clashing, overlap=ov)
    assert (r["conformer"], r["mode"], r["n_candidates"], r["n_passing"], r["n_dropped"]) == (0, 1, 5, 2, 0) and r["fraction"] == 4.99 / 10.0
    r = rule(v, clashing=clashing, overlap=ov, min_fraction=0.5)  # 5.0 >= 0.5 * 10.0 stays, 4.99 and 4.0 go: nothing that passes is left
    assert (r["n_candidates"], r["n_passing"], r["n_dropped"]) == (3, 0, 2) and r["passes"] is False and r["value"] == 10.0
    r = rule(v, clashing=clashing, overlap=[[2.0, 0.0, 1.0], [0.0, 0.0, 1.0]], min_fraction=0.5)
    assert (r["conformer"], r["mode"]) == (2, 0)
    r = rule(v, clashing=clashing, overlap=ov, min_fraction=1.0)
    assert (r["conformer"], r["mode"], r["n_candidates"], r["n_dropped"]) == (0, 0, 1, 4)
    # the product is a float64 product: 0.1 * 3.0 rounds above 0.3
    assert rule([[3.0, 0.3]], min_fraction=0.1)["n_dropped"] == 1 and rule([[3.0, 0.30000000000000004]], min_fraction=0.1)["n_dropped"] == 0
    # a slot dropped counts as dropped whatever its fit
    assert rule([[10.0, 1.0]], align_ok=[[True, False]], min_fraction=0.5)["n_dropped"] == 1


def test_rule_min_fitted_statuses_nan_and_nothing():
    v = [[9.0, 8.0, 7.0, 6.0]]
    r = rule(v, fitted=[[1, 2, 3, 3]], min_fitted=3)
    assert (r["conformer"], r["n_candidates"], r["value"]) == (2, 2, 7.0) and r["fraction"] == 7.0 / 9.0  # vbest is over the slots, not over the candidates
    r = rule(v, fitted=[[1, 2, 3, 3]])
    assert r["conformer"] == 0
    r = rule(v, align_ok=[[False, True, True, True]], clash_ok=[[True, False, True, True]])
    assert (r["conformer"], r["n_candidates"]) == (2, 2)
    r = rule([[np.nan, 2.0, 0.0, -1.0]])
    assert (r["conformer"], r["n_candidates"], r["vbest"], r["n_dropped"]) == (1, 1, 2.0, 0)  # NaN, 0 and a negative value are no candidates
    for nothing in (rule([[0.0, 0.0]]), rule([[np.nan, np.nan]]), rule(v, scored=False), rule(v, align_ok=np.zeros((1, 4), bool)), rule(v, fitted=np.zeros((1, 4)))):
        assert (nothing["conformer"], nothing["mode"], nothing["passes"], nothing["n_candidates"], nothing["n_passing"]) == (-1, -1, False, 0, 0)
        assert np.isnan(nothing["value"]) and np.isnan(nothing["fraction"])
    assert rule(v, scored=False)["n_dropped"] == 0 and rule(v, scored=False, min_fraction=1.0)["n_dropped"] == 0


# ---------------------------------------------------------------------------------------------------------------- the chain on the fixture
@lru_cache(maxsize=None)
def fixture_chain():
    """Per ligand of modes_set_6oim_c8 the chain at modes 1 and 4 over all 8 conformers (one cache of slot rows per ligand: 13 x 8 x (1 + 4)
    = 520 candidate rows counted per search, 416 distinct), and whether the default pose - the best conformer, mode 0 - passes."""
    from pharmaconet_amd.constants import weights_vector
    from pharmaconet_amd.pocket import PocketAtoms

    model, lib, weights, _ = load_golden("set_6oim_c8")
    w7 = weights_vector(weights)
    pocket = PocketAtoms.from_pdb(GOLDEN / "pocket_6oim.pdb", centers=model.node_centers)
    x = np.load(GOLDEN / "modes_set_6oim_c8.npz")
    out = []
    for r, i in enumerate(x["index"]):
        rec = lib.unpack(int(i))
        C, nl = int(x["n_conf"][r]), int(np.count_nonzero(x["levels"][r] != 0xFE))
        levels = x["levels"][r, :nl].astype(np.int64)
        cache = {}
        one, four = (psr.chain(model, rec, w7, pocket, levels, x["values"][r], x["key"][r], m, 8, cache=cache) for m in (1, 4))
        best = int(np.argmax(x["values"][r, 0, :C]))  # (the smallest conformer with the largest maximum)
        d = cache[0, best]
        out.append(dict(index=int(i), C=C, best=best, default=bool(d["align_ok"] and d["clash_ok"] and d["clashing"] == 0), one=one, four=four))
    return out


def test_chain_counts_on_the_fixture():
    hits = fixture_chain()
    assert len(hits) == 13 and all(h["C"] == 8 for h in hits)  # no hit is left out
    counts = [sum(h["default"] for h in hits), sum(h["one"]["passes"] for h in hits), sum(h["four"]["passes"] for h in hits)]
    frac4 = sorted(h["four"]["fraction"] for h in hits if h["four"]["passes"])
    frac1 = sorted(h["one"]["fraction"] for h in hits if h["one"]["passes"])
    print(f"hits with a passing pose, of 13: default pose {counts[0]}, all conformers at mode 0 {counts[1]}, all conformers at modes 0 to 3 {counts[2]}; "
          f"fraction of the best total: median {np.median(frac4):.3f} (mode 0 only: {np.median(frac1):.3f}), lowest {frac4[0]:.3f}")
    assert counts == [2, 4, 7]
    assert abs(np.median(frac4) - 0.952) < 5e-4 and abs(np.median(frac1) - 0.978) < 5e-4 and abs(frac4[0] - 0.153) < 5e-4
    for h in hits:
        assert h["one"]["n_candidates"] == 8 and h["four"]["n_candidates"] == 32  # every slot of the fixture scores and fits
        if h["default"]:  # the stated consequence
            assert (h["one"]["conformer"], h["one"]["mode"]) == (h["best"], 0) == (h["four"]["conformer"], h["four"]["mode"]) and h["four"]["fraction"] == 1.0
        if h["one"]["passes"]:  # more modes never lose a passing pose, and never choose a worse one
            assert h["four"]["passes"] and h["four"]["value"] >= h["one"]["value"]
    by = {h["index"]: h for h in hits}
    print(f"ligand 110: overlap of the default pose {by[110]['four']['rows'][0, by[110]['best']]['overlap']:.3g}, of the search's choice at mode 0 "
          f"{by[110]['one']['rows'][by[110]['one']['mode'], by[110]['one']['conformer']]['overlap']:.3g}")


def test_chain_decisions_stand_clear_of_their_thresholds():
    hits = fixture_chain()
    rows = sum(len(h[k]["rows"]) for h in hits for k in ("one", "four"))
    margin = min(s["margin"] for h in hits for s in h["four"]["rows"].values())
    print(f"smallest clash margin over {rows} candidate rows: {margin:.3g} (bar {MARGIN})")
    assert rows == 520 and margin >= MARGIN
    worst, equal = np.inf, 0
    for h in hits:
        for k in ("one", "four"):
            r = h[k]
            if r["passes"]:
                continue
            chosen = r["overlap"][r["mode"], r["conformer"]]
            for (m, c), s in r["rows"].items():
                if (m, c) == (r["mode"], r["conformer"]):
                    continue
                if s["overlap"] == chosen:
                    equal += 1
                else:
                    worst = min(worst, abs(s["overlap"] - chosen) / chosen)
    print(f"hits without a passing pose: {equal} overlaps bit-equal to the chosen one, every other at a relative gap of at least {worst:.3g} (bar {GAP})")
    assert worst >= GAP


# ---------------------------------------------------------------------------------------------------------------- the Python layer
def test_fitting_checks_the_search_arguments_before_anything_runs():
    from pharmaconet_amd.engine import ScreeningResult

    res = ScreeningResult(scores=None, status=None, first=0)
    for kw, word in ((dict(min_fraction=0.5), "min_fraction"), (dict(min_fitted=2), "min_fitted"), (dict(search=0, min_fraction=0.5, min_fitted=2), "min_fitted"),
                     (dict(search=9), "search"), (dict(search=-1), "search")):
        with pytest.raises(ValueError, match=word):
            res.fitting(4, **kw)
    with pytest.raises(ValueError, match="refinement"):  # (as before)
        res.fitting(4, search=4, restraint=0.1)


@pytest.mark.parametrize("flags", (
    ["--pose_search", "p.csv"],  # needs --explain K
    ["--explain", "5", "--pose_search", "p.csv", "--pose_search_modes", "0"],
    ["--explain", "5", "--pose_search", "p.csv", "--pose_search_modes", "9"],
    ["--explain", "5", "--pose_search", "p.csv", "--pose_min_fraction", "1.5"],
    ["--explain", "5", "--pose_search", "p.csv", "--pose_min_fraction", "nan"],
))
def test_cli_rejects_pose_search_flags_that_do_not_fit(flags, tmp_path, capsys):
    """Refused by the parser, before the model or the library is read (neither file exists)."""
    from pharmaconet_amd.screening import main

    with pytest.raises(SystemExit) as e:
        main(["-p", str(tmp_path / "none.pm"), "-d", str(tmp_path / "none.pmxlib"), "-o", str(tmp_path / "out.csv"), *flags])
    assert e.value.code == 2
    assert "--pose" in capsys.readouterr().err
    assert not (tmp_path / "out.csv").exists()
