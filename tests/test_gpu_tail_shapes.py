"""Both term-by-term tail arms of the score pass at every lane shape. A rough table cell is evaluated with `exact_value`
(csrc/pmx_screen_tables.h): always for a self item, for a pair item when the call's type weights are more than PMX_TAILS_RATIO apart
(`item_finish<TAILS>`, ligand_kernel<G, false, true>). Both arms diverge by lane - the rough flag is per lane, item_finish holds a ballot
behind a branch - and every kernel is compiled once per lane count G = 1 ... 64. tests/test_gpu_pair_tails.py and tests/test_gpu_tails.py
sweep the arms at 8 conformers (and 1), which pins the tables' accuracy; the small libraries here (tests/tail_cases.py) pin each
instantiation's control flow, against `oracle_score`. Bars: test_gpu_parity.py's 2e-6, and test_gpu_tails.py's 1.8e-6 between the default
and the term-by-term table phase."""

import numpy as np
import pytest

from conftest import rel_err
from tail_cases import FLOOR, PAIR_SHAPE_SETS, SELF_SHAPES, SHAPES, WEIGHT_SETS, _Shim, pair_shape_cases, self_shape_cases

pytestmark = pytest.mark.gpu

RTOL = 2e-6  # where the oracle's score is above FLOOR


def _screen(shim, lib, weights=None):
    from pharmaconet_amd import engine

    res = engine.screen(shim, lib, weights=weights)
    return res.scores.cpu().numpy(), res.status.cpu().numpy(), engine.last_score_stats()["n_exact_values"]


@pytest.mark.parametrize("wname,sigma_min_to", PAIR_SHAPE_SETS)
@pytest.mark.parametrize("conformers", SHAPES)
def test_pair_tail_arm_at_every_lane_shape(conformers, wname, sigma_min_to, monkeypatch):
    """ligand_kernel<G, false, true>: six cluster pairs of the rescaled fixture model (where the tabulated tail alone is off by 1e-5), one
    heavy item swept through its tails beside light items that pass. Statuses, 2e-6 against the oracle, items evaluated term by term - and
    with PMX_PAIR_TAILS=0 other bits on a record that is mostly that one tail item: the arm is taken, and it is what the score rests on."""
    cases = pair_shape_cases(wname, sigma_min_to, conformers)
    assert len(cases) == 6 and all(c.valid.all() for c in cases)
    n_scores, n_tail = sum(len(c.ref) for c in cases), sum(int(c.mostly_tail.sum()) for c in cases)
    assert 10 * n_tail >= n_scores
    wdict = WEIGHT_SETS[wname]
    worst, worst_off, n_exactv, n_differ = 0.0, 0.0, 0, 0
    for c in cases:
        shim = _Shim(c.flat)
        got, status, nv = _screen(shim, c.lib, wdict)
        assert np.all(status == 0), (c.a, c.b)
        n_exactv += nv
        worst = max(worst, float(rel_err(got, c.ref).max()))
        monkeypatch.setenv("PMX_PAIR_TAILS", "0")
        off, _, _ = _screen(shim, c.lib, wdict)
        monkeypatch.delenv("PMX_PAIR_TAILS")
        worst_off = max(worst_off, float(rel_err(off, c.ref).max()))
        n_differ += int((got.view(np.uint32) != off.view(np.uint32))[c.mostly_tail].sum())
    print(f"C={conformers} [{wname}, sigma_min {sigma_min_to}] {n_scores} scores, {n_tail} of them mostly one tail item ({n_differ} of those change "
          f"with the arm); {n_exactv} items term by term; max rel err {worst:.2e} (tabulated tails alone, PMX_PAIR_TAILS=0: {worst_off:.2e})")
    assert worst <= RTOL
    assert n_exactv > 0
    assert n_differ > 0, "no mostly-tail score depends on the arm: the shape shows nothing"


@pytest.mark.parametrize("conformers", SELF_SHAPES)
def test_self_tail_arm_at_every_lane_shape(conformers, monkeypatch):
    """item<..., SELF> -> exact_value: two-node ligands of the three clusters with the most subset pairs, swept to 5 A beyond the table
    range, against the oracle and against the term-by-term table phase (PMX_TREE_FLAGS=8)."""
    worst, worst_vs_exact, n_checked, n_slow = 0.0, 0.0, 0, 0
    for c in self_shape_cases(conformers):
        shim = _Shim(c.flat)
        got, status, nv = _screen(shim, c.lib)
        got = got.astype(np.float64)
        assert np.all(status == 0), c.a
        n_slow += nv
        sel = c.ref > FLOOR
        assert sel.any(), c.a
        assert np.all(got[~sel] <= FLOOR * (1 + RTOL)), "scores the oracle puts below the floor"
        err = rel_err(got[sel], c.ref[sel])
        worst = max(worst, float(err.max()))
        n_checked += int(sel.sum())
        monkeypatch.setenv("PMX_TREE_FLAGS", "8")
        exact, _, _ = _screen(shim, c.lib)
        monkeypatch.delenv("PMX_TREE_FLAGS")
        worst_vs_exact = max(worst_vs_exact, float(rel_err(got[sel], exact.astype(np.float64)[sel]).max()))
        assert err.max() <= RTOL, f"cluster {c.a}: max rel err {err.max():.3e} at oracle score {c.ref[sel][err.argmax()]:.3e}"
    print(f"C={conformers}: {n_checked} scores above {FLOOR:g}; max rel err vs oracle {worst:.2e}, default vs term-by-term {worst_vs_exact:.2e}; "
          f"{n_slow} self items evaluated term by term")
    assert n_slow > 0  # the sweep reaches the flagged cells
    assert worst_vs_exact <= 1.8e-6  # (test_gpu_tails.py's bar, for the reason it gives)
