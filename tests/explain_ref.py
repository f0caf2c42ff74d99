"""A NumPy restatement of what `pmx_explain` answers, for the explain tests: the score tables of one ligand
(match_utils.py:9-122 and the cluster-distance prefilter of graph_match.py:263-268), a leaf's total `path_score`, and the
reference's tree (tree.py:15-104) walked in `root_tree.iteration()` order for the per-conformer maxima and the first leaf that
reaches each. float64 arithmetic throughout: totals agree with the reference's float32 / float64 mix to about 1e-7."""

from __future__ import annotations

import itertools

import numpy as np

NONE = -1


def ligand_levels(model, rec) -> list[int]:
    """The record's clusters that have a candidate model cluster, in priority order, at most 20 (graph_match.py:87-88,124-137)."""
    flat = model.flat
    ends = rec["cluster_end"]
    out = []
    for q in range(int(rec["n_clusters"])):
        s0 = int(ends[q - 1]) if q else 0
        tm = int(np.bitwise_or.reduce(rec["typemask"][s0 : int(ends[q])])) if int(ends[q]) > s0 else 0
        if any(int(t) & tm for t in flat.cluster_typemask):
            out.append(q)
    return out[:20]


def candidates(model, rec, lc: int) -> list[int]:
    ends = rec["cluster_end"]
    s0 = int(ends[lc - 1]) if lc else 0
    tm = int(np.bitwise_or.reduce(rec["typemask"][s0 : int(ends[lc])])) if int(ends[lc]) > s0 else 0
    return [m for m, t in enumerate(model.flat.cluster_typemask) if int(t) & tm]


class Tables:
    """Self and pair scores of one ligand against one model, computed on demand (float64 [C] vectors; -1 = no match)."""

    def __init__(self, model, rec, weights7):
        self.flat = model.flat
        self.rec = rec
        self.w = np.asarray(weights7, dtype=np.float64)
        self.C = int(rec["n_conf"])
        self.pos = rec["xyz"].astype(np.float32).transpose(0, 2, 1)  # [n, C, 3]
        ends = rec["cluster_end"]
        self.ranges = [(int(ends[q - 1]) if q else 0, int(ends[q])) for q in range(int(rec["n_clusters"]))]
        cn = np.asarray(self.flat.cluster_nodes, dtype=np.uint64)
        cn = cn.reshape(cn.shape[0], -1)
        nm = self.flat.num_nodes
        self.members = [[m for m in range(nm) if (int(cn[a, m // 64]) >> (m % 64)) & 1] for a in range(cn.shape[0])]
        self._cache = {}

    def _matches(self, lc, mc):
        out = []
        s0, s1 = self.ranges[lc]
        for u in range(s0, s1):
            tm = int(self.rec["typemask"][u])
            ms = [m for m in self.members[mc] if (tm >> int(self.flat.node_type[m])) & 1]
            if ms:
                out.append((u, ms, np.array([self.w[int(self.flat.node_type[m])] for m in ms], dtype=np.float32).astype(np.float64)))
        return out

    def _dist(self, u, v):
        d = self.pos[u] - self.pos[v]
        return np.linalg.norm(d, axis=-1).astype(np.float64)  # (float32 like ligand.py's edge distances)

    def _term(self, a, b):
        (u, m1, w1), (v, m2, w2) = a, b
        d = self._dist(u, v)
        pairs = list(itertools.product(m1, m2))
        means = np.array([self.flat.edge_mean[p, q] for p, q in pairs], dtype=np.float64)[:, None]
        stds = np.array([self.flat.edge_std[p, q] for p, q in pairs], dtype=np.float64)[:, None]
        wts = (w1[:, None] * w2[None, :]).reshape(-1)
        z = (d[None, :] - means) / stds
        like = (wts / stds[:, 0]) @ np.exp(-0.5 * z**2)
        npass = (np.abs(z) < 2.0).sum(axis=0)
        return like / len(pairs), npass < len(pairs) * 0.5  # (normalize_coeff * score_coeff = 1 / num_match)

    def self_score(self, lc, mc):
        key = ("s", lc, mc)
        if key not in self._cache:
            ml = self._matches(lc, mc)
            acc = np.zeros(self.C)
            for a, b in itertools.combinations(ml, 2):
                acc += self._term(a, b)[0]
            self._cache[key] = acc
        return self._cache[key]

    def _center_size(self, lc):
        s0, s1 = self.ranges[lc]
        p = self.pos[s0:s1].astype(np.float32)  # [k, C, 3]
        ctr = p.mean(axis=0)
        size = np.linalg.norm(p - ctr[None], axis=-1).max(axis=0)
        return ctr, size

    def pair_score(self, lc1, mc1, lc2, mc2):
        key = ("p", lc1, mc1, lc2, mc2)
        if key not in self._cache:
            c1, s1 = self._center_size(lc1)
            c2, s2 = self._center_size(lc2)
            ld = np.linalg.norm(c1 - c2, axis=-1).astype(np.float64)
            md = float(np.sqrt(((self.flat.cluster_center[mc1] - self.flat.cluster_center[mc2]) ** 2).sum()))
            ms = float(self.flat.cluster_size[mc1] + self.flat.cluster_size[mc2])
            if np.min(np.abs(ld - md) - (s1 + s2).astype(np.float64)) > ms:
                out = np.full(self.C, -1.0)
            else:
                l1, l2 = self._matches(lc1, mc1), self._matches(lc2, mc2)
                acc = np.zeros(self.C)
                fails = np.zeros(self.C)
                for a, b in itertools.product(l1, l2):
                    v, f = self._term(a, b)
                    acc += v
                    fails += f
                out = np.where(fails <= len(l1) * len(l2) * 0.5, acc, -1.0)
            self._cache[key] = out
        return self._cache[key]


def path_score(model, record, weights7, levels, key, c: int, tables: Tables | None = None) -> float:
    """Total of the leaf `key` (model cluster or -1 per level) for conformer c: self terms plus pair terms; NaN when a pair on
    the path is not > 0 for c (the leaf does not hold c)."""
    T = tables or Tables(model, record, weights7)
    matched = [(int(levels[l]), int(key[l])) for l in range(len(levels)) if int(key[l]) != NONE]
    tot = 0.0
    for j, (lc, mc) in enumerate(matched):
        tot += T.self_score(lc, mc)[c]
        for lc0, mc0 in matched[:j]:
            v = T.pair_score(lc0, mc0, lc, mc)[c]
            if not v > 0:
                return float("nan")
            tot += v
    return tot


def first_max_key(leaves, C: int):
    """The key rule: per conformer the maximum over (key, {c: score}) leaves given in iteration order, and the first leaf whose
    score equals it (0 / None where no leaf scores > 0) - what a strict `>` update in `_run_average` keeps."""
    best = np.zeros(C)
    keys: list = [None] * C
    for key, sc in leaves:
        for c, v in sc.items():
            if v > best[c]:
                best[c] = v
                keys[c] = tuple(key)
    return best, keys


def tree_leaves(model, record, weights7, tables: Tables | None = None, limit: int = 200_000):
    """The reference's tree (tree.py:55-104) for one ligand, its leaves in `iteration()` order as (key, {conformer: score}).
    Raises RuntimeError past `limit` nodes."""
    T = tables or Tables(model, record, weights7)
    lv = ligand_levels(model, record)
    cand = [candidates(model, record, lc) for lc in lv]
    C = T.C
    leaves = []
    count = [0]

    def dfs(level, path, scores):  # path: [(lc, mc | -1)], scores: {c: total} of this node; returns max_num_matches + matched
        count[0] += 1
        if count[0] > limit:
            raise RuntimeError("tree too large")
        matched_here = bool(path) and path[-1][1] != NONE
        if level == len(lv):
            leaves.append(([m for _, m in path], dict(scores)))
            return int(matched_here)
        lc = lv[level]
        nm = sum(1 for _, m in path if m != NONE)
        mx = 0
        children = 0
        for mc in cand[level]:
            ok = {}
            for c, t in scores.items():
                good = True
                acc = 0.0
                for lc0, mc0 in path:
                    if mc0 == NONE:
                        continue
                    v = T.pair_score(lc0, mc0, lc, mc)[c]
                    if not v > 0:
                        good = False
                        break
                    acc += v
                if good:
                    ok[c] = (t + T.self_score(lc, mc)[c]) + acc
            if ok:
                children += 1
                mx = max(mx, dfs(level + 1, path + [(lc, mc)], ok))
        if children == 0 or nm + mx < 5:
            mx = max(mx, dfs(level + 1, path + [(lc, NONE)], scores))
        return mx + int(matched_here)

    if lv:
        dfs(0, [], {c: 0.0 for c in range(C)})
    return lv, leaves
