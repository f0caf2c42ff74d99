"""CPU side of the hotspot feature (`pmx_hotspots`, `pmx_fingerprint_*`): the NumPy restatement of tests/hotspot_ref.py against the
reference's recorded totals (tests/golden/attribution_<set>.npz), the Tanimoto and leader rules on hand-made bit sets, the command
line's flag checks, and the C entry points' argument checks."""

import ctypes

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from explain_ref import Tables
from hotspot_ref import bits_to_words, hotspots, leaders, matched_members, tanimoto
from test_attribution_cpu import ATTRIBUTION_SETS, attribution_rows

BAR = 2e-6  # of the leaf's total: the project's bar (tests/test_gpu_attribution.py)


def fp_of(*nodes):
    bits = np.zeros(256, dtype=bool)
    bits[list(nodes)] = True
    return bits_to_words(bits)


@pytest.mark.parametrize("name", ATTRIBUTION_SETS)
def test_restated_shares_add_up_to_the_reference_total(name):
    """On the reference's own leaves: the model-side shares sum to the recorded total within 2e-6 of it, none is negative, and none lies
    outside the members of the model clusters the key matches."""
    from pharmaconet_amd.constants import weights_vector

    model, lib, weights, _ = load_golden(name)
    w7 = weights_vector(weights)
    seen = 0
    for i, c, key, lv, _, _, total in attribution_rows(np.load(GOLDEN / f"attribution_{name}.npz")):
        rec = lib.unpack(i)
        T = Tables(model, rec, w7)
        out = hotspots(model, rec, w7, lv, key, c, T)
        assert out["valid"], (name, i)
        assert abs(out["share"].sum() - total) <= BAR * total, (name, i, out["share"].sum(), total)
        assert (out["share"] >= 0).all()
        inside = matched_members(T, key)
        assert (out["share"][~inside] == 0).all() and (out["terms"][~inside] == 0).all()
        assert (out["passes"] <= out["terms"]).all()
        assert out["terms"].sum() % 2 == 0  # (every inner term is counted once per side)
        seen += total > 0
    assert seen > 0


def test_tanimoto_rule():
    empty, a, b = fp_of(), fp_of(1, 2, 3, 200), fp_of(3, 200, 255)
    sim = tanimoto(np.stack([empty, a, b, fp_of(64, 128)]), np.stack([empty, a, b]))
    assert sim.dtype == np.float32 and sim.shape == (4, 3)
    assert sim[0, 0] == 1.0  # empty against empty
    assert sim[0, 1] == 0.0 and sim[1, 0] == 0.0
    assert sim[1, 1] == 1.0 and sim[2, 2] == 1.0  # identical
    assert sim[1, 2] == np.float32(2) / np.float32(5)  # bits 3 and 200 (word 3) of {1, 2, 3, 200, 255}
    assert (sim[3] == 0.0).all()  # disjoint


def test_leader_rule():
    # a ~ b ~ c at 0.5, a !~ c: c must not follow b into a's cluster
    a, b, c = fp_of(0, 1, 2, 3), fp_of(1, 2, 3, 4, 5), fp_of(2, 3, 4, 5, 6)
    s = tanimoto(np.stack([a, b, c]), np.stack([a, b, c]))
    assert s[0, 1] >= 0.5 and s[1, 2] >= 0.5 and s[0, 2] < 0.5
    lead, of = leaders(np.stack([a, b, c]), 0.5, 2048)
    assert lead.tolist() == [0, 2] and of.tolist() == [0, 0, 2]
    # empty joins empty; identical joins at threshold 1; a bit in word 3 tells two rows apart
    rows = np.stack([fp_of(), fp_of(), fp_of(10), fp_of(10), fp_of(10, 250), fp_of(250)])
    lead, of = leaders(rows, 1.0, 2048)
    assert lead.tolist() == [0, 2, 4, 5] and of.tolist() == [0, 0, 2, 2, 4, 5]
    # disjoint rows are all leaders until max_leaders is reached; later ones still join an existing leader
    rows = np.stack([fp_of(1), fp_of(2), fp_of(3), fp_of(2), fp_of(4), fp_of(1)])
    lead, of = leaders(rows, 0.7, 2)
    assert lead.tolist() == [0, 1] and of.tolist() == [0, 1, -1, 1, -1, 0]
    lead, of = leaders(rows, 0.7, 1)
    assert lead.tolist() == [0] and of.tolist() == [0, -1, -1, -1, -1, 0]
    lead, of = leaders(np.zeros((0, 4), dtype=np.uint64), 0.7, 8)
    assert len(lead) == 0 and len(of) == 0


@pytest.mark.parametrize("flags", (
    ["--hotspots", "h.csv"],  # needs --explain K
    ["--diverse", "5"],  # needs --diverse_out
    ["--diverse", "0", "--diverse_out", "d.csv"],
    ["--diverse_out", "d.csv"],  # needs --diverse K
    ["--diverse_pool", "100"],
    ["--diverse", "5", "--diverse_out", "d.csv", "--diverse_pool", "0"],
    ["--diverse", "5", "--diverse_out", "d.csv", "--diverse_pool", "65537"],
    ["--diverse", "5", "--diverse_out", "d.csv", "--diverse_threshold", "0"],
    ["--diverse", "5", "--diverse_out", "d.csv", "--diverse_threshold", "1.5"],
))
def test_cli_rejects_flags_that_do_not_fit(flags, tmp_path, capsys):
    """Refused by the parser, before the model or the library is read (neither file exists)."""
    from pharmaconet_amd.screening import main

    with pytest.raises(SystemExit) as e:
        main(["-p", str(tmp_path / "none.pm"), "-d", str(tmp_path / "none.pmxlib"), "-o", str(tmp_path / "out.csv"), *flags])
    assert e.value.code == 2
    assert "--" in capsys.readouterr().err
    assert not (tmp_path / "out.csv").exists()


def test_entry_points_check_their_arguments_without_a_gpu():
    import __graft_entry__ as entry

    entry.build()
    from pharmaconet_amd import _ffi

    lib = _ffi.load()
    none = [None] * 7
    assert lib.pmx_hotspots(None, None, None, None, None, None, 1, *none, None) == 1 and b"null" in lib.pmx_last_error()
    fake = ctypes.create_string_buffer(256)  # (stands for a model and a library: no call below gets as far as reading one)
    w = (ctypes.c_float * _ffi.NUM_TYPES)(*([1.0] * _ffi.NUM_TYPES))
    addr = ctypes.addressof(fake)
    assert lib.pmx_hotspots(addr, addr, w, None, None, None, 0, *none, None) == 0  # n = 0 succeeds
    assert lib.pmx_hotspots(addr, addr, w, None, None, None, 65537, *none, None) == 1 and b"65536" in lib.pmx_last_error()
    assert lib.pmx_hotspots(addr, addr, w, None, None, None, 1, *none, None) == 1 and b"null" in lib.pmx_last_error()
    assert lib.pmx_fingerprint_tanimoto(None, 65537, None, 1, None, 0, None) == 1 and b"65536" in lib.pmx_last_error()
    assert lib.pmx_fingerprint_tanimoto(None, 1, None, 65537, None, 0, None) == 1
    assert lib.pmx_fingerprint_tanimoto(None, 0, None, 5, None, 0, None) == 0  # nothing to write
    assert lib.pmx_fingerprint_tanimoto(None, 1, None, 1, None, 0, None) == 1 and b"null" in lib.pmx_last_error()
    for thr, cap, n in ((0.0, 8, 1), (-0.5, 8, 1), (1.5, 8, 1), (float("nan"), 8, 1), (0.7, 0, 1), (0.7, 2049, 1), (0.7, 8, 65537)):
        assert lib.pmx_fingerprint_leaders(addr, n, thr, cap, addr, addr, addr, 0, None) == 1, (thr, cap, n)
    assert lib.pmx_fingerprint_leaders(None, 1, 0.7, 8, None, None, None, 0, None) == 1 and b"null" in lib.pmx_last_error()
