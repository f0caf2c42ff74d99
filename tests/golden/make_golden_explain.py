#!/usr/bin/env python3
"""Mint tests/golden/explain_<set>.npz by running the REFERENCE's tree search on ligands of the golden sets.

Run in the build container only (needs /root/reference, like make_golden.py, whose reference import, FakeLigand and extract it
reuses; never on the GPU box):

    python tests/golden/make_golden_explain.py

Per chosen ligand of a set (the molecules come back from `<set>_mols.npz`, the same ones make_golden.py packed):
  * index            the ligand's index in the set's library
  * levels           the ligand cluster behind each tree level, as its index in the packed record's cluster list (0xFE past nl)
  * scores           the reference's per-conformer vector of `_run_average` (graph_match.py:103-109), 0 past C
  * key              per conformer the key (`ClusterMatchTree.key`, tree.py:129-137) of the first leaf in `root_tree.iteration()` order
                     whose score for that conformer equals its maximum - the leaf a strict `>` update keeps - as model-cluster indices
                     (`model.node_clusters` order), 0xFF for None; all 0xFF where the maximum is 0
  * gap              (max - best score of a leaf with a different key) / max: 0 for an exact tie, 1 where no other leaf holds the
                     conformer or the maximum is 0
Ligands are chosen on the set's `n_tree` column: mostly small trees, a few at the large end (the reference enumerates every node).
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

import make_golden as mg  # noqa: E402  (imports the reference)

from pharmaconet_amd.constants import CLUSTER_PRIORITY, MAX_CONFORMERS, MAX_LEVELS  # noqa: E402
from pharmaconet_amd.library import LigandFeatures  # noqa: E402

SETS = {  # set -> (small trees, large trees, largest tree taken)
    "set_6oim_c8": (14, 4, 150_000),
    "set_6oim_c1": (12, 3, 150_000),
    "set_6oim_c64": (8, 2, 60_000),
    "set_c21_c8": (14, 4, 150_000),
    "set_6oim_c8_weights": (10, 3, 150_000),
    "set_s64_c8": (6, 2, 60_000),
}


def load_mols(name):
    d = np.load(HERE / f"{name}_mols.npz")
    mols, o = [], 0
    for t, shp in zip(json.loads(str(d["topology"])), d["shapes"]):
        cnt = int(np.prod(shp))
        feats = [(f[0], f[1] if isinstance(f[1], int) else tuple(f[1]), f[2] if isinstance(f[2], int) else tuple(f[2])) for f in t["features"]]
        mols.append(LigandFeatures(t["z"], t["nbrs"], feats, d["positions"][o : o + cnt].reshape(tuple(int(x) for x in shp))))
        o += cnt
    return mols


def choose(n_tree, small, large, cap):
    order = np.argsort(n_tree, kind="stable")
    nontrivial = [int(i) for i in order if n_tree[i] >= 3 and n_tree[i] <= 3000]
    step = max(1, len(nontrivial) // max(small, 1))
    picked = nontrivial[::step][:small]
    big = [int(i) for i in order[::-1] if 3000 < n_tree[i] <= cap][:large]
    zero = [int(i) for i in order if n_tree[i] == 0][:1]  # a ligand without levels
    return sorted(set(picked + big + zero))


def explain_one(model, mol, weights):
    lig = mg.FakeLigand(mol)
    C = lig.num_conformers
    levels = np.full(MAX_LEVELS, 0xFE, np.uint8)
    scores = np.zeros(MAX_CONFORMERS)
    key = np.full((MAX_CONFORMERS, MAX_LEVELS), 0xFF, np.uint8)
    gap = np.ones(MAX_CONFORMERS)
    gm = mg.GraphMatcher(model, lig, weights)
    if len(gm.ligand_graph.node_clusters) == 0:
        return C, levels, scores, key, gap
    gm.setup()
    if len(gm.ligand_cluster_list) == 0:
        return C, levels, scores, key, gap
    # the packed record's cluster order (library.pack_clustered_ligand: priority_fn, stable)
    cl = mg.extract(lig.graph)
    order = sorted(range(len(cl.clusters)), key=lambda i: (CLUSTER_PRIORITY[cl.cluster_types[i]][0], -len(cl.clusters[i]),
                                                           CLUSTER_PRIORITY[cl.cluster_types[i]][1], cl.cluster_key_atom[i]))
    packed_pos = {g: r for r, g in enumerate(order)}
    graph_index = {id(c): i for i, c in enumerate(lig.graph.node_clusters)}
    for lv, lc in enumerate(gm.ligand_cluster_list):
        levels[lv] = packed_pos[graph_index[id(lc)]]
    mc_index = {id(m): i for i, m in enumerate(model.node_clusters)}
    root = gm.run_tree()
    best_leaf = [None] * C
    leaves = list(root.iteration())
    for leaf in leaves:  # _run_average's loop, remembering the leaf each strict `>` keeps
        for c, s in leaf.pair_scores.items():
            if s > scores[c]:
                scores[c] = s
                best_leaf[c] = leaf
    assert abs(float(np.mean(scores[:C])) - gm._run_average(root)) <= 1e-12 * max(1.0, abs(gm._run_average(root)))
    keys = {}
    for c in range(C):
        if best_leaf[c] is None:
            continue
        k = tuple(0xFF if m is None else mc_index[id(m)] for m in best_leaf[c].key)
        keys[c] = k
        key[c, : len(k)] = k
    for c, k in keys.items():
        other = -np.inf
        for leaf in leaves:
            s = leaf.pair_scores.get(c)
            if s is not None and s > other and tuple(0xFF if m is None else mc_index[id(m)] for m in leaf.key) != k:
                other = s
        gap[c] = 1.0 if other == -np.inf else max(0.0, (scores[c] - other) / scores[c])
    return C, levels, scores, key, gap


def main():
    for name, (small, large, cap) in SETS.items():
        t0 = time.time()
        d = np.load(HERE / f"{name}.npz")
        weights = json.loads(str(d["weights"]))
        model = mg.RefModel.load(str(HERE / f"{str(d['model'])}.pm"))
        mols = load_mols(name)
        idx = choose(d["n_tree"], small, large, cap)
        rows = [explain_one(model, mols[i], weights) for i in idx]
        np.savez_compressed(
            HERE / f"explain_{name}.npz",
            index=np.array(idx, dtype=np.int32),
            n_conf=np.array([r[0] for r in rows], dtype=np.int32),
            levels=np.stack([r[1] for r in rows]),
            scores=np.stack([r[2] for r in rows]),
            key=np.stack([r[3] for r in rows]),
            gap=np.stack([r[4] for r in rows]),
        )
        print(f"explain_{name}: {len(idx)} ligands (trees up to {int(d['n_tree'][idx].max())} nodes), {time.time() - t0:.1f}s", flush=True)


if __name__ == "__main__":
    main()
