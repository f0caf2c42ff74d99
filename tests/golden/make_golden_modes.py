#!/usr/bin/env python3
"""Mint tests/golden/modes_<set>.npz: the REFERENCE's tree search on ligands of the golden sets, its leaves ranked per conformer.

Run in the build container only (it imports the reference through make_golden.py, like make_golden_constrained.py, whose
`reference_leaves` and `choose` it shares; never on the GPU box):

    python tests/golden/make_golden_modes.py [set ...]

Per conformer c the ranked list holds the leaves of `root.iteration()` whose pair_scores give c a score > 0, by descending score, equal
scores in iteration order. Per chosen ligand, with M = 8:
  * index, n_conf, levels   the ligand, C, the ligand cluster behind each level (as explain_<set>.npz)
  * values [8][64]          the m-th entry's score for conformer c; 0 past the list's end
  * key    [8][64][20]      its key as model-cluster indices, 0xFF for None; all 0xFF past the list's end
  * gap    [8][64]          (entry m - entry m + 1) / entry m, the ninth entry included; 1 where there is no next entry
  * n_positive [64]         the length of the list, capped at 255
Only data is written.
"""

from __future__ import annotations

import json
import sys
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))

import make_golden as mg  # noqa: E402  (imports the reference)
from make_golden_constrained import SETS, choose, reference_leaves  # noqa: E402
from make_golden_explain import load_mols  # noqa: E402

from pharmaconet_amd.constants import MAX_CONFORMERS, MAX_LEVELS  # noqa: E402

M = 8
TIE = 1e-5  # the GPU test compares an entry by its total instead of its key when its own gap or its predecessor's is <= TIE
POOL = 3  # ligands looked at per ligand kept: those with the fewest near ties stay
# Sets in which NO ligand has a conformer with 2 .. 7 scoring leaves: every ligand with a tree of 3 .. 30 000 nodes is ranked here and the
# absence asserted (set_s64_c8: 60 ligands, shortest list 9 leaves; set_l110_c8: 48 ligands, shortest list 42). Their fixtures hold
# lists of 8 and more only; the short lists of the five other sets pin the entries past a list's end.
NO_SHORT_LIST = ("set_s64_c8", "set_l110_c8")
SHARED = 3  # rows of explain_<set>.npz (small trees) taken along, so that mode 0 is pinned to that fixture


def rank(leaves, C):
    values = np.zeros((M, MAX_CONFORMERS))
    key = np.full((M, MAX_CONFORMERS, MAX_LEVELS), 0xFF, np.uint8)
    gap = np.ones((M, MAX_CONFORMERS))
    n_positive = np.zeros(MAX_CONFORMERS, np.int32)
    for c in range(C):
        have = [(s, o, k) for o, (k, ps) in enumerate(leaves) for s in [ps.get(c)] if s is not None and s > 0]
        have.sort(key=lambda e: (-e[0], e[1]))  # descending score, iteration order among equals
        n_positive[c] = min(len(have), 255)
        for m, (s, _, k) in enumerate(have[:M]):
            values[m, c] = s
            key[m, c, : len(k)] = k
            if m + 1 < len(have):
                gap[m, c] = max(0.0, (s - have[m + 1][0]) / s)
    return values, key, gap, n_positive


def loose_entries(values, gap):
    """(entries with value > 0 whose own gap or predecessor's gap is <= TIE, entries with value > 0)."""
    pos = values > 0
    near = gap <= TIE
    near[1:] |= gap[:-1] <= TIE
    return int((pos & near).sum()), int(pos.sum())


def mint(name, small, small_cap, large, cap):
    d = np.load(HERE / f"{name}.npz")
    weights = json.loads(str(d["weights"]))
    model = mg.RefModel.load(str(HERE / f"{str(d['model'])}.pm"))
    mols = load_mols(name)
    chosen = choose(d["n_tree"], POOL * small, small_cap, large, cap)
    if name in NO_SHORT_LIST:
        chosen = [int(i) for i in np.argsort(d["n_tree"], kind="stable") if 3 <= d["n_tree"][i] <= 30_000]
    ex = np.load(HERE / f"explain_{name}.npz") if (HERE / f"explain_{name}.npz").exists() else None
    if ex is not None:
        chosen = sorted(set(chosen) | set([int(i) for i in ex["index"] if 3 <= d["n_tree"][i] <= small_cap][:SHARED]))
    rows = []
    for i in chosen:
        C, levels, leaves, _ = reference_leaves(model, mols[i], weights)
        if not leaves:
            continue
        values, key, gap, n_positive = rank(leaves, C)
        row = dict(index=i, C=C, levels=levels, values=values, key=key, gap=gap, n_positive=n_positive)
        row["deep"] = any(sum(m != 0xFF for m in k) >= 5 for k, _ in leaves)
        row["few"] = bool(((n_positive[:C] > 1) & (n_positive[:C] < M)).any())
        row["many"] = bool((n_positive[:C] >= M).any())
        row["shared"] = ex is not None and i in ex["index"]
        row["small"] = int(d["n_tree"][i]) <= 2000  # (a tree the tests' NumPy restatement walks)
        row["loose"], row["pos"] = loose_entries(values, gap)
        if row["shared"]:
            r = int(np.flatnonzero(ex["index"] == i)[0])
            assert np.array_equal(values[0], ex["scores"][r]) and np.array_equal(key[0], ex["key"][r]), (name, i)
            assert np.array_equal(levels, ex["levels"][r])
        rows.append(row)

    def bites(rs):  # the fixture cannot be passed by a one-mode walker or an unpruned one, holds a tree small enough to restate, and pins mode 0 to the explain fixture
        need = ("many", "deep", "small") + (("few",) if name not in NO_SHORT_LIST else ()) + (("shared",) if ex is not None else ())
        return all(any(r[p] for r in rs) for p in need)

    def capped(rs):  # at most half of the positive entries may be compared by total instead of by key
        return 2 * sum(r["loose"] for r in rs) <= sum(r["pos"] for r in rs)

    # other ligands, not a looser cap: of the pool, the rows with the largest share of near ties leave until the cap holds and the
    # fixture has the size asked for
    assert bites(rows), name
    assert name not in NO_SHORT_LIST or not any(r["few"] for r in rows), name
    while not capped(rows) or len(rows) > small + large + SHARED:
        for r in sorted(rows, key=lambda r: -r["loose"] / max(r["pos"], 1)):
            rest = [q for q in rows if q is not r]
            if bites(rest):
                rows = rest
                break
        else:
            raise AssertionError((name, "no ligand left to drop"))
    n_loose, n_pos, shared = sum(r["loose"] for r in rows), sum(r["pos"] for r in rows), sum(r["shared"] for r in rows)
    assert bites(rows) and capped(rows) and n_pos > 0, (name, n_loose, n_pos)
    np.savez_compressed(
        HERE / f"modes_{name}.npz",
        index=np.array([r["index"] for r in rows], dtype=np.int32),
        n_conf=np.array([r["C"] for r in rows], dtype=np.int32),
        levels=np.stack([r["levels"] for r in rows]),
        values=np.stack([r["values"] for r in rows]),
        key=np.stack([r["key"] for r in rows]),
        gap=np.stack([r["gap"] for r in rows]),
        n_positive=np.stack([r["n_positive"] for r in rows]),
    )
    return len(rows), n_loose, n_pos, shared


def main():
    for name in sys.argv[1:] or SETS:
        t0 = time.time()
        n_rows, n_loose, n_pos, shared = mint(name, *SETS[name])
        print(f"modes_{name}: {n_rows} ligands, {n_loose} of {n_pos} entries within {TIE} of a neighbour, {shared} shared with explain_{name}, {time.time() - t0:.1f}s", flush=True)


if __name__ == "__main__":
    main()
