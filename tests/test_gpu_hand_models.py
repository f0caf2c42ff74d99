"""The cases of tests/model_cases.py on the GPU (-m gpu), each against the CPU oracle: models whose edge matrix is not symmetric (A), cells
of two pass windows (B), the floats at the ends of the 2-sigma windows (C) and a model of 256 nodes and 128 clusters (D). Scores are held to
the project's parity tolerance, `RTOL + 6e-8` (tests/test_gpu_model_upload.py); where the oracle says exactly 0 the engine says exactly 0,
so the zero / non-zero pattern along a sweep is the oracle's float for float; every case gives the same bits twice in a row.
tests/test_model_cases_cpu.py shows without a GPU that each case reaches what it is run for.

Measured on an MI355X, the largest relative deviation from the oracle per family: A1 2.1e-7 (term by term 1.2e-7), A2 6.4e-7 (1.2e-7),
A3 6.4e-8, B1 2.3e-7, B2 1.2e-7, B3 3.4e-7, C 3.6e-7, D 8.4e-8; attribution totals against the explained maxima 5.0e-8. `n_exact_cells`
(counted per lane): B1 139264 at C = 1 and 4352 at C = 64, B2 0, B3 290 to 18270 per cell."""

import numpy as np
import pytest

import model_cases as mc
from conftest import rel_err
from tail_cases import _Shim
from test_gpu_parity import RTOL

pytestmark = pytest.mark.gpu

TOL = RTOL + 6e-8
ARMS = {"default": {}, "term_by_term": {"PMX_TREE_FLAGS": "8"}, "overflow_pass": {"PMX_SLICE_KB": "8"}}


def run(case, monkeypatch=None, env=None):
    """(float32 scores as float64, score statistics) of the case through the public path, twice: status 0 everywhere, the same bits."""
    from pharmaconet_amd import engine

    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    try:
        model = _Shim(case.flat)  # pmx_model_create on first use
        first = engine.screen(model, case.lib)
        stats = engine.last_score_stats()
        again = engine.screen(_Shim(case.flat), case.lib)
        a, b = first.scores.cpu().numpy(), again.scores.cpu().numpy()
        assert np.all(first.status.cpu().numpy() == 0) and np.all(again.status.cpu().numpy() == 0), case.name
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), case.name
    finally:
        for k in env or {}:
            monkeypatch.delenv(k)
    return a.astype(np.float64), stats


def check(case, got):
    """Exactly 0 where the oracle is, within TOL elsewhere. Returns the largest relative deviation."""
    ref = case.ref
    zero = ref == 0
    assert np.all(got[zero] == 0.0), (case.name, "non-zero where the oracle is zero at rows", np.flatnonzero(zero & (got != 0))[:8].tolist())
    assert np.all(got[~zero] > 0.0), (case.name, "zero where the oracle is not at rows", np.flatnonzero(~zero & (got == 0))[:8].tolist())
    if zero.all():
        return 0.0
    err = rel_err(got[~zero], ref[~zero])
    assert err.max() <= TOL, (case.name, f"max rel err {err.max():.3e} at row {np.flatnonzero(~zero)[err.argmax()]}, oracle {ref[~zero][err.argmax()]:.6e}")
    return float(err.max())


# ------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("arm", tuple(ARMS))
def test_a1_pairs_of_an_asymmetric_model(arm, oracle, monkeypatch):
    """`asym3` created through the public path, against ligands of two one-node clusters in both cluster orders: edge (m, n) for the node of
    the earlier level against the node of the later one. The transposed model's scores differ by up to 1.7 on two rows of three."""
    worst = max(check(case, run(case, monkeypatch, ARMS[arm])[0]) for case in mc.a1_cases())
    print(f"A1 {arm}: max rel err vs oracle {worst:.2e}")


@pytest.mark.parametrize("arm", tuple(ARMS))
def test_a2_self_entries_of_an_asymmetric_model(arm, oracle, monkeypatch):
    """`asym3` reduced to one cluster, against two-node ligands in both node orders: edge (m, n) for the earlier node against the later."""
    worst = max(check(case, run(case, monkeypatch, ARMS[arm])[0]) for case in mc.a2_cases())
    print(f"A2 {arm}: max rel err vs oracle {worst:.2e}")


def test_a3_golden_ligands_against_asymmetric_golden_models(oracle):
    for case in mc.a3_cases():
        print(f"A3 {case.name}: max rel err vs oracle {check(case, run(case)[0]):.2e}")


@pytest.mark.parametrize("k", (0, 1), ids=[s[1] for s in mc.A3_SETS[:2]])  # (the 110-node model's row calls take 11 s for its 4 ligands)
def test_a3_explain_attribution_and_hotspots_agree_on_an_asymmetric_model(k, oracle):
    """The per-conformer maxima give back the score (test_gpu_explain.check_against_score_pass; the first ligand's keys
    are restated on the CPU as well; the first 16 ligands of a set), the attribution of every ligand's best leaf adds up to the explained total within 2e-6 (test_gpu_attribution's bar), and the
    hotspot totals are the attribution totals bit for bit (README) - on models where the SWAP arm of csrc/pmx_rows.hip reads another edge
    than the plain one."""
    from test_gpu_attribution import BAR
    from test_gpu_explain import check_against_score_pass

    case = mc.a3_cases()[k]
    model = _Shim(case.flat)
    rows = np.arange(min(len(case.lib), 16))
    ex = check_against_score_pass(model, case.lib, None, rows, n_path=1)
    at = ex.attribution(model, case.lib)
    hs = ex.hotspots(model, case.lib)
    assert len(at) == int((ex.status == 0).sum()) == len(rows)
    worst = 0.0
    for r, i in enumerate(at.rows):
        cm = float(ex.conf_max[i][ex.best_conformer[i]])
        assert at.status[r] == 0 and abs(float(at.total[r]) - cm) <= BAR * cm, (case.name, i, at.total[r], cm)
        worst = max(worst, abs(float(at.total[r]) - cm) / cm)
    assert np.array_equal(hs.rows, at.rows) and np.array_equal(hs.status, at.status)
    assert np.array_equal(hs.total.view(np.uint64), at.total.view(np.uint64)), case.name
    print(f"A3 {case.name}: attribution total vs explained maximum {worst:.2e}")


# ------------------------------------------------------------------------------------------------ B
def test_b1_the_gap_inside_a_cell(oracle):
    """`gap_in_cell`, cell [4.0, 4.125): pass / gap / pass with both transitions between neighbouring floats, one float per score (C = 1) and
    64 per mean (C = 64: one conformer on the wrong side moves a mean by 1/64 of 0.26)."""
    c1, c64 = mc.b1_cases()
    got, stats = run(c1)
    worst = check(c1, got)  # (the zero / non-zero pattern float for float)
    assert stats["n_exact_cells"] > 0
    got64, stats64 = run(c64)
    worst = max(worst, check(c64, got64))
    assert stats64["n_exact_cells"] > 0
    print(f"B1: max rel err vs oracle {worst:.2e}; n_exact_cells {stats['n_exact_cells']} (C = 1), {stats64['n_exact_cells']} (C = 64)")


def test_b2_the_gap_on_a_cell_edge(oracle):
    """`gap_on_cell_edge`: the same two windows with the gap starting at a cell's first float - every cell holds one window, no item is
    counted term by term."""
    c1, c64 = mc.b2_cases()
    got, stats = run(c1)
    worst = check(c1, got)
    got64, stats64 = run(c64)
    worst = max(worst, check(c64, got64))
    print(f"B2: max rel err vs oracle {worst:.2e}; n_exact_cells {stats['n_exact_cells']}, {stats64['n_exact_cells']}")
    assert stats["n_exact_cells"] == 0 and stats64["n_exact_cells"] == 0  # pmx.h: the counter is for pass sets that are not an interval


def test_b3_the_complex_cells_of_the_fixture_model(oracle):
    worst = 0.0
    for c1, c64 in mc.b3_cases():
        for case in (c1, c64):
            got, stats = run(case)
            worst = max(worst, check(case, got))
            assert stats["n_exact_cells"] > 0, case.name
            print(case.name, "n_exact_cells", stats["n_exact_cells"], "decided" if case.aim[-1] else "reached")
    print(f"B3: max rel err vs oracle {worst:.2e}")


# ------------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("model", mc.C_MODELS)
def test_c_window_ends_to_the_float(model, oracle, monkeypatch):
    """Four floats either side of wlo and whi of every edge of 32 one-pair and 16 several-pair functions: the tabulated windows (the cell
    from d, lo <= d <= hi) and the term-by-term test (|d - mean| <= T) both turn where the oracle's `abs((d - mean) / std) < 2` turns."""
    worst = 0.0
    single, multi = mc.c_functions(model)
    for fn in single + multi:
        got, _ = run(fn.case)
        exact, _ = run(fn.case, monkeypatch, ARMS["term_by_term"])
        worst = max(worst, check(fn.case, got), check(fn.case, exact))
        assert np.array_equal(got > 0, exact > 0), fn.case.name
    print(f"C {model}: max rel err vs oracle {worst:.2e}")


# ------------------------------------------------------------------------------------------------ D
def test_d_a_model_at_the_limits_of_the_header(oracle):
    """256 nodes in four node words and 128 clusters in two cluster words (the oracle takes this size: its own bounds are the header's), the
    last cluster of node 255 and a node of word 0; ligands whose masks make clusters 0, 63, 64 and 127 candidates."""
    case = mc.d_case()
    print(f"D: max rel err vs oracle {check(case, run(case)[0]):.2e}")
