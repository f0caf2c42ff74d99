"""NumPy restatement of the pose search (`pmx_pose_search`, include/pmx.h): the selection rule on per-slot arrays, and the whole chain on one
record - tests/align_ref.py fits every slot, tests/clash_ref.py checks every fit, the rule chooses.

A hit has slots (m, c): binding mode m < M of conformer c < S, v = value[m, c] the leaf total `pmx_explain_modes` reports.
  vbest      the largest v > 0 over the slots (0 when there is none, or when the hit was not scored)
  candidate  the hit was scored; v > 0; the fit of the slot's row is OK with at least `min_fitted` fitted nodes; the clash check of the fit
             is OK; v >= min_fraction * vbest (a float64 product)
  dropped    scored, v > 0, and v >= min_fraction * vbest does not hold - whatever the fit says
  passes     a candidate with at most `max_clashing` points that have a clashing pair
  choice     among the passing candidates the largest v, then the lowest c, then the lowest m; when none passes, among the candidates the
             smallest overlap, then the largest v, then the lowest c, then the lowest m; without a candidate: none (-1, -1, NaN)
Comparisons are on the float64 values as given: equal means equal bits (there is no -0.0 among totals and overlaps)."""

from __future__ import annotations

import numpy as np

import align_ref
import clash_ref
from explain_ref import NONE, Tables

NO_MATCH = 0xFF


def choose(value, align_ok, fitted, clash_ok, clashing, overlap, scored=True, max_clashing=0, min_fitted=1, min_fraction=0.0) -> dict:
    """The rule on arrays of shape [M, S]. Returns conformer, mode, passes, n_candidates, n_passing, n_dropped, value, fraction, vbest and the
    boolean masks `candidate` and `passing`."""
    value = np.asarray(value, dtype=np.float64)
    M, S = value.shape
    positive = np.zeros((M, S), bool) if not scored else value > 0  # (a NaN is not)
    vbest = float(value[positive].max()) if positive.any() else 0.0
    worth = np.zeros((M, S), bool)
    worth[positive] = value[positive] >= np.float64(min_fraction) * np.float64(vbest)
    dropped = positive & ~worth
    candidate = worth & np.asarray(align_ok, bool) & (np.asarray(fitted) >= min_fitted) & np.asarray(clash_ok, bool)
    passing = candidate & (np.asarray(clashing) <= max_clashing)
    out = dict(conformer=-1, mode=-1, passes=False, n_candidates=int(candidate.sum()), n_passing=int(passing.sum()), n_dropped=int(dropped.sum()),
               value=float("nan"), fraction=float("nan"), vbest=vbest, candidate=candidate, passing=passing)
    if not candidate.any():
        return out
    if passing.any():
        order = sorted((-value[m, c], c, m) for m, c in zip(*np.nonzero(passing)))
        _, c, m = order[0]
    else:
        ov = np.asarray(overlap, dtype=np.float64)
        order = sorted((ov[m, c], -value[m, c], c, m) for m, c in zip(*np.nonzero(candidate)))
        _, _, c, m = order[0]
    out.update(conformer=int(c), mode=int(m), passes=bool(passing[m, c]), value=float(value[m, c]), fraction=float(value[m, c] / vbest))
    return out


def unique(fit, gate=1e-4) -> bool:
    """Is the fit's rotation determined by its pairs? tests/test_gpu_align.py's gate: gap >= 1e-4 E0. Where it is not - one matched
    cluster, whose nodes share one target centroid, gives S = 0 and leaves the rotation free - `pmx_align` takes the identity (the lowest
    index among equal eigenvalues) and NumPy's eigensolver whatever it takes: two correct fits, two different poses."""
    return fit["n_pairs"] > 0 and fit["gap"] >= gate * fit["E0"]


def slot(model, rec, w7, pocket, levels, key, c, tables=None, centers=None, node_radius=1.0, tolerance=0.5, contact=4.5, method="horn", motion=None) -> dict:
    """One row: the fit of `key` (uint8, 0xFF for None, or ints with NONE) at conformer c and the clash check of the fitted nodes.
    align_ok, fitted, clash_ok, clashing, overlap, margin, and `fit` / `clash`: the two restatements' own answers. `motion`: an (R, t) to
    check in place of the restatement's own - for a row whose rotation is not `unique`, the motion of the fit under test."""
    nl = len(levels)
    k = [NONE if int(v) in (NO_MATCH, NONE) else int(v) for v in np.asarray(key).reshape(-1)[:nl]]
    fit = align_ref.align(model, rec, w7, levels, k, int(c), tables, method, centers)
    out = dict(align_ok=bool(fit["valid"]), fitted=int(fit.get("n_nodes", 0)), clash_ok=False, clashing=0, overlap=float("nan"), margin=float("inf"), fit=fit, clash=None)
    if not fit["valid"]:
        return out
    nodes = rec["xyz"][:, :, int(c)].astype(np.float32)
    R, t = (fit["R"], fit["t"]) if motion is None else motion
    cl = clash_ref.clash_row(pocket.xyz, pocket.radius, pocket.group, nodes, np.float32(node_radius), R, t, tolerance, contact)
    out.update(clash_ok=cl["status"] == 0, clashing=int(cl["counts"][1]), overlap=float(cl["overlap"]), margin=float(cl["margin"]), clash=cl)
    return out


def chain(model, rec, w7, pocket, levels, values, keys, modes, conf_stride, max_clashing=0, min_fitted=1, min_fraction=0.0, node_radius=1.0, tolerance=0.5,
          contact=4.5, cache=None, centers=None) -> dict:
    """The whole search on one scored record: `values` [>= modes][64] and `keys` [>= modes][64][20] as `pmx_explain_modes` lays them out.
    Every slot with v > 0 is fitted and checked (`cache`: a dict that keeps a slot's row between calls). Returns `choose`'s answer with
    `rows` - {(m, c): slot} - and `overlap` [M, S]. Rows cut to the record's conformers (an `engine.ModeSet`'s) are taken as well."""
    M, S = int(modes), int(conf_stride)
    v = np.zeros((M, S))
    given = np.asarray(values, dtype=np.float64)[:M, :S]
    v[:, : given.shape[1]] = given
    T = Tables(model, rec, w7)
    Y = align_ref.node_centers(model) if centers is None else centers
    cache = {} if cache is None else cache
    a_ok, fitted, c_ok = np.zeros((M, S), bool), np.zeros((M, S), np.int64), np.zeros((M, S), bool)
    clashing, overlap = np.zeros((M, S), np.int64), np.full((M, S), np.nan)
    rows = {}
    for m in range(M):
        for c in range(S):
            if not v[m, c] > 0:
                continue
            if (m, c) not in cache:
                cache[m, c] = slot(model, rec, w7, pocket, levels, keys[m][c], c, T, Y, node_radius, tolerance, contact)
            r = rows[m, c] = cache[m, c]
            a_ok[m, c], fitted[m, c], c_ok[m, c], clashing[m, c], overlap[m, c] = r["align_ok"], r["fitted"], r["clash_ok"], r["clashing"], r["overlap"]
    out = choose(v, a_ok, fitted, c_ok, clashing, overlap, True, max_clashing, min_fitted, min_fraction)
    out.update(rows=rows, overlap=overlap)
    return out
