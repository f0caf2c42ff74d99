"""CPU side of the pose feature (`pmx_align`): the NumPy restatement of tests/align_ref.py checked against itself - its SVD fit against its
quaternion fit - and the C entry point: declared, bound, exported, and checking its arguments."""

import ctypes
import subprocess

import numpy as np
import pytest

import align_ref
from conftest import GOLDEN, REPO, load_golden
from explain_ref import NONE, Tables, candidates, ligand_levels


def explained_rows(name):
    """(library index, conformer, levels, key) of the reference's recorded explanations of a set (tests/golden/explain_<set>.npz): the key of
    every ligand's best conformer."""
    x = np.load(GOLDEN / f"explain_{name}.npz")
    for r, i in enumerate(x["index"]):
        C = int(x["n_conf"][r])
        nl = int(np.count_nonzero(x["levels"][r] != 0xFE))
        c = int(np.argmax(x["scores"][r, :C]))
        key = x["key"][r, c, :nl].astype(np.int64)
        key[key == 0xFF] = NONE
        yield int(i), c, x["levels"][r, :nl].astype(np.int64), key


@pytest.mark.parametrize("name", ("set_6oim_c8", "set_c21_c8", "set_6oim_c1"))
def test_svd_fit_and_quaternion_fit_agree(name):
    """The first 48 ligands, conformer 0, every level matched to its first candidate (a key need not be a leaf), and the recorded
    explanations at their best conformer: the two methods' sse within 1e-12 E0, both rotations proper, sse = rn + spread."""
    from pharmaconet_amd.constants import weights_vector

    model, lib, weights, _ = load_golden(name)
    w7 = weights_vector(weights)
    Y = align_ref.node_centers(model)
    assert np.array_equal(Y, model.node_centers)
    rows = []
    for i in range(min(48, len(lib))):
        rec = lib.unpack(i)
        if rec["n_conf"]:
            lv = ligand_levels(model, rec)
            rows.append((i, 0, lv, [candidates(model, rec, q)[0] for q in lv]))
    rows += list(explained_rows(name))
    worst, fitted = 0.0, 0
    for i, c, lv, key in rows:
        rec = lib.unpack(i)
        T = Tables(model, rec, w7)
        a = align_ref.align(model, rec, w7, lv, key, c, T, "svd", Y)
        b = align_ref.align(model, rec, w7, lv, key, c, T, "horn", Y)
        assert a["valid"] and b["valid"] and a["n_pairs"] == b["n_pairs"]
        if a["n_pairs"] == 0:
            continue
        fitted += 1
        for f in (a, b):
            assert abs(np.linalg.det(f["R"]) - 1.0) <= 1e-12 and np.abs(f["R"] @ f["R"].T - np.eye(3)).max() <= 1e-12
            assert abs(f["sse"] - (f["rn"] + f["spread"])) <= 1e-12 * f["E0"]
        worst = max(worst, abs(a["sse"] - b["sse"]) / a["E0"])
        assert abs(a["sse"] - b["sse"]) <= 1e-12 * a["E0"], (name, i, a["sse"], b["sse"], a["E0"])
    assert fitted > 0
    print(f"{name}: svd against quaternion, sse difference of E0: {worst:.3g} over {fitted} rows")


def test_header_declares_pmx_align():
    text = (REPO / "include" / "pmx.h").read_text()
    assert "int pmx_align(const pmx_model *model, const pmx_library *lib, const float weights[PMX_NUM_TYPES]," in text
    assert "const double *node_center_dev" in text


def test_ffi_binds_pmx_align():
    from pharmaconet_amd import _ffi

    restype, argtypes = _ffi.SIGNATURES["pmx_align"]
    assert restype is ctypes.c_int and len(argtypes) == 16 and argtypes[7] is ctypes.c_uint32


def test_library_exports_pmx_align_and_checks_its_arguments():
    import __graft_entry__ as entry

    entry.build()
    from pharmaconet_amd import _ffi

    syms = subprocess.run(["nm", "-D", "--defined-only", str(_ffi.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert " T pmx_align\n" in syms
    lib = _ffi.load()
    none = [None] * 7
    assert lib.pmx_align(None, None, None, None, None, None, None, 1, *none, None) == 1 and b"null" in lib.pmx_last_error()
    fake = ctypes.create_string_buffer(256)  # (stands for a model and a library: neither call below gets as far as reading one)
    w = (ctypes.c_float * _ffi.NUM_TYPES)(*([1.0] * _ffi.NUM_TYPES))
    addr = ctypes.addressof(fake)
    assert lib.pmx_align(addr, addr, w, None, None, None, None, 0, *none, None) == 0  # n = 0 succeeds
    assert lib.pmx_align(addr, addr, w, None, None, None, None, 65537, *none, None) == 1 and b"65536" in lib.pmx_last_error()
    assert lib.pmx_align(addr, addr, w, None, addr, addr, addr, 1, *([addr] * 7), None) == 1 and b"null" in lib.pmx_last_error()  # no node centres
