"""A NumPy restatement of what `pmx_attribute` answers, for the attribution tests, on top of tests/explain_ref.py's `Tables` (`_matches`,
`_term`, `_center_size`): for a (record, conformer, key) the matrix of self and pair entries, the failing node pairs, whether the key is a
leaf that holds the conformer, the node shares and the total. float64 arithmetic throughout, like explain_ref.py: it agrees with the
reference's float32 / float64 mix to about 1e-7."""

from __future__ import annotations

import itertools

import numpy as np

from explain_ref import NONE, Tables, candidates


def prefilter_margin(T: Tables, model, lc1: int, mc1: int, lc2: int, mc2: int) -> float:
    """graph_match.py:263-268 as a margin in Angstrom: min over conformers of |ligand cluster distance - model cluster distance| - ligand
    cluster sizes, minus the model cluster sizes. The pair is rejected iff it is > 0."""
    flat = model.flat
    c1, s1 = T._center_size(lc1)
    c2, s2 = T._center_size(lc2)
    ld = np.linalg.norm(c1 - c2, axis=-1).astype(np.float64)
    md = float(np.sqrt(((flat.cluster_center[mc1] - flat.cluster_center[mc2]) ** 2).sum()))
    ms = float(flat.cluster_size[mc1] + flat.cluster_size[mc2])
    return float(np.min(np.abs(ld - md) - (s1 + s2).astype(np.float64))) - ms


def attribution(model, rec, weights7, levels, key, c: int, tables: Tables | None = None) -> dict:
    """entry [nl, nl] (diagonal and upper triangle; -1 = no match), fails [nl, nl], valid, node [n_nodes] (half of every term a node is part
    of) and total (walker order) of the leaf `key` (model cluster or -1 per level) for conformer c. A match that is not a candidate of its
    level makes the row invalid and counts as None; with a conformer the ligand does not have nothing is computed."""
    T = tables or Tables(model, rec, weights7)
    nl, n = len(levels), int(rec["n_nodes"])
    entry = np.zeros((nl, nl))
    fails = np.zeros((nl, nl), dtype=np.int64)
    node = np.zeros(n)
    key = [int(k) for k in key] + [NONE] * (nl - len(key))
    valid = 0 <= c < T.C and all(k == NONE for k in key[nl:])
    use = []
    for l in range(nl):
        if key[l] == NONE:
            continue
        if key[l] in candidates(model, rec, int(levels[l])):
            use.append(l)
        else:
            valid = False
    if not 0 <= c < T.C:
        return dict(entry=entry, fails=fails, valid=False, node=np.full(n, np.nan), total=float("nan"))
    lists = {l: T._matches(int(levels[l]), key[l]) for l in use}
    for l in use:
        for a, b in itertools.combinations(lists[l], 2):
            v = float(T._term(a, b)[0][c])
            entry[l, l] += v
            node[a[0]] += 0.5 * v
            node[b[0]] += 0.5 * v
    for l1, l2 in itertools.combinations(use, 2):
        acc, nf = 0.0, 0
        for a, b in itertools.product(lists[l1], lists[l2]):
            v, f = T._term(a, b)
            acc += float(v[c])
            nf += int(f[c])
            node[a[0]] += 0.5 * float(v[c])
            node[b[0]] += 0.5 * float(v[c])
        fails[l1, l2] = nf
        dead = prefilter_margin(T, model, int(levels[l1]), key[l1], int(levels[l2]), key[l2]) > 0 or nf > len(lists[l1]) * len(lists[l2]) * 0.5
        entry[l1, l2] = -1.0 if dead else acc
        if not entry[l1, l2] > 0:
            valid = False
    total = 0.0
    for j, l in enumerate(use):
        total = (total + entry[l, l]) + sum(entry[l0, l] for l0 in use[:j])
    if not valid:
        return dict(entry=entry, fails=fails, valid=False, node=np.full(n, np.nan), total=float("nan"))
    return dict(entry=entry, fails=fails, valid=True, node=node, total=float(total))
