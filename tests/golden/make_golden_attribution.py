#!/usr/bin/env python3
"""Mint tests/golden/attribution_<set>.npz by asking the REFERENCE what the explaining leaf of a ligand's best conformer is made of.

Run in the build container only (needs /root/reference, like make_golden.py, whose reference import and FakeLigand it reuses, and
make_golden_explain.py, whose `load_mols` and level mapping it reuses; never on the GPU box):

    python tests/golden/make_golden_attribution.py

For every ligand of `explain_<set>.npz` (same order), at conformer c = the first conformer with the largest maximum and under the key
the reference's tree search recorded for c:
  * index, conformer   the ligand's index in the set's library and c
  * key                the key as model-cluster indices (0xFF for None) - explain_<set>.npz's key[c]
  * levels             the ligand cluster behind each tree level, as in explain_<set>.npz
  * entry              float64 [20, 20]: for matched levels l1 <= l2 the reference's `matching_pair_scores_dict[lc1, lc2][mc1, mc2][c]` as it
                       stands (the self entry on the diagonal, -1 for no match), 0 elsewhere
  * node               float64 [64]: per node of the packed record, half of the reference's own `scoring_matching_self([match_u, match_v], C)[c]`
                       - which is term(u, v) - summed over every node pair (u, v) that enters an entry above, in record node order
  * total              the leaf's score for c as the reference's tree holds it (`leaf.pair_scores[c]`), 0 where the key is all None
Only data is written.
"""

from __future__ import annotations

import itertools
import json
import sys
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import make_golden as mg  # noqa: E402  (imports the reference)
from make_golden_explain import SETS, load_mols  # noqa: E402

from pmnet.scoring.match_utils import scoring_matching_self  # noqa: E402

from pharmaconet_amd.constants import CLUSTER_PRIORITY, MAX_LEVELS  # noqa: E402

MAX_NODES = 64


def attribute_one(model, mol, weights, c, key, levels):
    lig = mg.FakeLigand(mol)
    C = lig.num_conformers
    entry = np.zeros((MAX_LEVELS, MAX_LEVELS))
    node = np.zeros(MAX_NODES)
    gm = mg.GraphMatcher(model, lig, weights)
    if len(gm.ligand_graph.node_clusters) == 0:
        return entry, node, 0.0
    gm.setup()
    if len(gm.ligand_cluster_list) == 0:
        return entry, node, 0.0
    # the packed record's cluster and node order (library.pack_clustered_ligand: priority_fn, stable)
    cl = mg.extract(lig.graph)
    order = sorted(range(len(cl.clusters)), key=lambda i: (CLUSTER_PRIORITY[cl.cluster_types[i]][0], -len(cl.clusters[i]),
                                                           CLUSTER_PRIORITY[cl.cluster_types[i]][1], cl.cluster_key_atom[i]))
    packed_pos = {g: r for r, g in enumerate(order)}
    record_node = {}
    for g in order:
        for u in cl.clusters[g]:
            record_node[u] = len(record_node)
    graph_index = {id(cl_): i for i, cl_ in enumerate(lig.graph.node_clusters)}
    for lv, lc in enumerate(gm.ligand_cluster_list):
        assert levels[lv] == packed_pos[graph_index[id(lc)]]
    matched = [(lv, gm.ligand_cluster_list[lv], model.node_clusters[int(key[lv])]) for lv in range(len(gm.ligand_cluster_list)) if key[lv] != 0xFF]
    psd = gm.matching_pair_scores_dict
    for (l1, lc1, mc1), (l2, lc2, mc2) in itertools.combinations_with_replacement(matched, 2):
        entry[l1, l2] = psd[lc1, lc2][mc1, mc2][c]
        list1, list2 = gm.node_match_dict[lc1, mc1], gm.node_match_dict[lc2, mc2]
        pairs = itertools.combinations(list1, 2) if l1 == l2 else itertools.product(list1, list2)
        for mu, mv in pairs:
            t = float(scoring_matching_self([mu, mv], C)[c])
            node[record_node[mu[0].index]] += 0.5 * t
            node[record_node[mv[0].index]] += 0.5 * t
    total = 0.0
    if matched:
        mc_index = {id(m): i for i, m in enumerate(model.node_clusters)}
        want = tuple(int(k) for k in key[: len(gm.ligand_cluster_list)])
        for leaf in gm.run_tree().iteration():
            if tuple(0xFF if m is None else mc_index[id(m)] for m in leaf.key) == want:
                total = float(leaf.pair_scores[c])
                break
        else:
            raise AssertionError("the recorded key is not a leaf of the reference's tree")
    return entry, node, total


def main():
    for name in SETS:
        t0 = time.time()
        d = np.load(HERE / f"{name}.npz")
        x = np.load(HERE / f"explain_{name}.npz")
        weights = json.loads(str(d["weights"]))
        model = mg.RefModel.load(str(HERE / f"{str(d['model'])}.pm"))
        mols = load_mols(name)
        rows, conf, keys = [], [], []
        for r, i in enumerate(x["index"]):
            C = int(x["n_conf"][r])
            c = int(np.argmax(x["scores"][r, :C]))
            key = x["key"][r, c]
            rows.append(attribute_one(model, mols[int(i)], weights, c, key, x["levels"][r]))
            conf.append(c)
            keys.append(key)
        np.savez_compressed(
            HERE / f"attribution_{name}.npz",
            index=x["index"].astype(np.int32),
            conformer=np.array(conf, dtype=np.int32),
            key=np.stack(keys).astype(np.uint8),
            levels=x["levels"],
            entry=np.stack([r[0] for r in rows]),
            node=np.stack([r[1] for r in rows]),
            total=np.array([r[2] for r in rows]),
        )
        print(f"attribution_{name}: {len(rows)} ligands, {time.time() - t0:.1f}s", flush=True)


if __name__ == "__main__":
    main()
