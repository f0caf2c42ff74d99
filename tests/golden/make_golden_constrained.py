#!/usr/bin/env python3
"""Mint tests/golden/constrained_<set>.npz: the REFERENCE's tree search on ligands of the golden sets, its leaves filtered by a constraint.

Run in the build container only (it imports the reference through make_golden.py, like make_golden_explain.py, whose `load_mols`, level
mapping and key encoding it shares; never on the GPU box):

    python tests/golden/make_golden_constrained.py [set ...]

A constraint is up to 8 require groups (sets of model clusters, indices into `model.node_clusters`) and one exclude set; a leaf of
`root.iteration()` qualifies when its key holds a cluster of every group and none of the exclude set. Per chosen ligand the rows are
derived from its own unconstrained best key (the key of its best conformer):
  a  require the deepest matched cluster of that key (satisfied: that conformer's maximum is unchanged)
  b  exclude that cluster
  c  require a cluster that occurs in some leaf but not in that key (the largest such index)
  d  two groups, one of them holding two clusters: {deepest, the cluster of c} and {shallowest matched cluster of the key}
  e  require a cluster that is a candidate of no level (every maximum is 0)
Per row:
  * index, kind, n_conf, levels     the ligand, the letter above, C, the ligand cluster behind each level (as explain_<set>.npz)
  * n_require, require, exclude     the constraint as bit masks (bit a % 64 of word a / 64: model cluster a)
  * scores, key, gap                as explain_<set>.npz, over the QUALIFYING leaves only
  * unconstrained                   the per-conformer maxima over all leaves
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
from make_golden_explain import load_mols  # noqa: E402

from pharmaconet_amd.constants import CLUSTER_PRIORITY, MAX_CONFORMERS, MAX_LEVELS  # noqa: E402

MAX_GROUPS = 8
SETS = {  # set -> (small trees, their largest, large trees, their largest)
    "set_6oim_c8": (8, 3000, 2, 60_000),
    "set_6oim_c1": (8, 3000, 2, 60_000),
    "set_6oim_c64": (8, 3000, 1, 30_000),
    "set_c21_c8": (8, 3000, 2, 60_000),
    "set_6oim_c8_weights": (8, 3000, 1, 60_000),
    "set_s64_c8": (8, 3000, 1, 30_000),
    "set_l110_c8": (8, 8000, 1, 30_000),  # 86 clusters: masks reach the second word
}


def choose(n_tree, small, small_cap, large, cap):
    order = np.argsort(n_tree, kind="stable")
    nontrivial = [int(i) for i in order if 3 <= n_tree[i] <= small_cap]
    step = max(1, len(nontrivial) // max(small, 1))
    picked = nontrivial[::step][:small]
    big = [int(i) for i in order[::-1] if small_cap < n_tree[i] <= cap][:large]
    return sorted(set(picked + big))


def bits(clusters):
    w = np.zeros(2, np.uint64)
    for a in clusters:
        w[a // 64] |= np.uint64(1) << np.uint64(a % 64)
    return w


def qualifies(key, require, exclude):
    have = {m for m in key if m != 0xFF}
    return all(have & set(g) for g in require) and not (have & set(exclude))


def first_max(leaves, C, require, exclude):
    """_run_average's loop over the qualifying leaves: maxima, the key each strict `>` keeps, and the gap to another qualifying key."""
    scores = np.zeros(MAX_CONFORMERS)
    key = np.full((MAX_CONFORMERS, MAX_LEVELS), 0xFF, np.uint8)
    gap = np.ones(MAX_CONFORMERS)
    ok = [(k, ps) for k, ps in leaves if qualifies(k, require, exclude)]
    keys = {}
    for k, ps in ok:
        for c, s in ps.items():
            if s > scores[c]:
                scores[c] = s
                keys[c] = k
    for c, k in keys.items():
        key[c, : len(k)] = k
        other = -np.inf
        for k2, ps in ok:
            s = ps.get(c)
            if s is not None and s > other and k2 != k:
                other = s
        gap[c] = 1.0 if other == -np.inf else max(0.0, (scores[c] - other) / scores[c])
    return scores, key, gap


def reference_leaves(model, mol, weights):
    """(C, levels, [(key as model-cluster indices with 0xFF for None, pair_scores)] in root.iteration() order, candidate clusters of any level)."""
    lig = mg.FakeLigand(mol)
    C = lig.num_conformers
    levels = np.full(MAX_LEVELS, 0xFE, np.uint8)
    gm = mg.GraphMatcher(model, lig, weights)
    if len(gm.ligand_graph.node_clusters) == 0:
        return C, levels, [], set()
    gm.setup()
    if len(gm.ligand_cluster_list) == 0:
        return C, levels, [], set()
    cl = mg.extract(lig.graph)  # the packed record's cluster order (library.pack_clustered_ligand: priority_fn, stable)
    order = sorted(range(len(cl.clusters)), key=lambda i: (CLUSTER_PRIORITY[cl.cluster_types[i]][0], -len(cl.clusters[i]),
                                                           CLUSTER_PRIORITY[cl.cluster_types[i]][1], cl.cluster_key_atom[i]))
    packed_pos = {g: r for r, g in enumerate(order)}
    graph_index = {id(c): i for i, c in enumerate(lig.graph.node_clusters)}
    for lv, lc in enumerate(gm.ligand_cluster_list):
        levels[lv] = packed_pos[graph_index[id(lc)]]
    mc_index = {id(m): i for i, m in enumerate(model.node_clusters)}
    cand = {mc_index[id(m)] for lc in gm.ligand_cluster_list for m in gm.cluster_match_dict[lc]}  # (graph_match.py:124-137)
    root = gm.run_tree()
    leaves = [(tuple(0xFF if m is None else mc_index[id(m)] for m in leaf.key), dict(leaf.pair_scores)) for leaf in root.iteration()]
    return C, levels, leaves, cand


def constraints_of(leaves, C, cand, n_clusters):
    """The rows a - e of one ligand, from its unconstrained best key; [] for a ligand no leaf scores."""
    scores, key, _ = first_max(leaves, C, [], [])
    if scores.max() <= 0:
        return scores, []
    kb = [int(m) for m in key[int(np.argmax(scores[:C]))] if m != 0xFF]
    deepest, shallowest = kb[-1], kb[0]
    in_leaves = {m for k, ps in leaves if any(s > 0 for s in ps.values()) for m in k if m != 0xFF}
    others = sorted(in_leaves - set(kb))
    out = [("a", [[deepest]], []), ("b", [], [deepest])]
    if others:
        out.append(("c", [[others[-1]]], []))
        out.append(("d", [[deepest, others[-1]], [shallowest]], []))
    never = [a for a in range(n_clusters) if a not in cand]
    if never:
        out.append(("e", [[never[-1]]], []))
    return scores, out


def mint(name, small, small_cap, large, cap):
    d = np.load(HERE / f"{name}.npz")
    weights = json.loads(str(d["weights"]))
    model = mg.RefModel.load(str(HERE / f"{str(d['model'])}.pm"))
    mols = load_mols(name)
    K = len(model.node_clusters)
    rows = []
    deep = 0
    for i in choose(d["n_tree"], small, small_cap, large, cap):
        C, levels, leaves, cand = reference_leaves(model, mols[i], weights)
        if not leaves:
            continue
        deep += any(sum(m != 0xFF for m in k) >= 5 for k, _ in leaves)
        unc, cons = constraints_of(leaves, C, cand, K)
        for kind, require, exclude in cons:
            sc, key, gap = first_max(leaves, C, require, exclude)
            rows.append(dict(index=i, kind=kind, C=C, levels=levels, require=require, exclude=exclude, scores=sc, key=key, gap=gap, unc=unc))
    # the fixture cannot be passed by ignoring constraints
    for kind in "bc":
        rk = [r for r in rows if r["kind"] == kind]
        differs = [r for r in rk if not np.array_equal(r["scores"], r["unc"]) and r["scores"].max() > 0]
        assert 2 * len(differs) >= len(rk) > 0, (name, kind, len(differs), len(rk))
    assert all(np.array_equal(r["scores"], np.zeros(MAX_CONFORMERS)) for r in rows if r["kind"] == "e")
    assert all((r["scores"] <= r["unc"]).all() for r in rows)
    assert deep > 0, name
    if name == "set_l110_c8":
        assert any(r["kind"] == "b" and r["exclude"][0] >= 64 for r in rows) and any(r["kind"] == "c" and r["require"][0][0] >= 64 for r in rows)
    req = np.zeros((len(rows), MAX_GROUPS, 2), np.uint64)
    for r, row in enumerate(rows):
        for g, grp in enumerate(row["require"]):
            req[r, g] = bits(grp)
    np.savez_compressed(
        HERE / f"constrained_{name}.npz",
        index=np.array([r["index"] for r in rows], dtype=np.int32),
        kind=np.array([ord(r["kind"]) for r in rows], dtype=np.uint8),
        n_conf=np.array([r["C"] for r in rows], dtype=np.int32),
        levels=np.stack([r["levels"] for r in rows]),
        n_require=np.array([len(r["require"]) for r in rows], dtype=np.int32),
        require=req,
        exclude=np.stack([bits(r["exclude"]) for r in rows]),
        scores=np.stack([r["scores"] for r in rows]),
        key=np.stack([r["key"] for r in rows]),
        gap=np.stack([r["gap"] for r in rows]),
        unconstrained=np.stack([r["unc"] for r in rows]),
    )
    return len(rows), len({r["index"] for r in rows})


def main():
    for name in sys.argv[1:] or SETS:
        t0 = time.time()
        n_rows, n_lig = mint(name, *SETS[name])
        print(f"constrained_{name}: {n_rows} rows of {n_lig} ligands, {time.time() - t0:.1f}s", flush=True)


if __name__ == "__main__":
    main()
