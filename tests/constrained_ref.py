"""Constrained matching restated for the tests: the key rule of `explain_ref.first_max_key` over the leaves that qualify under a
constraint - require groups (each a set of model clusters, one of which the key must hold) and an exclude set (none of which it may) -
and the reading of tests/golden/constrained_<set>.npz (tests/golden/make_golden_constrained.py)."""

from __future__ import annotations

import numpy as np

from conftest import GOLDEN, load_golden
from explain_ref import NONE, first_max_key

CONSTRAINED_SETS = ("set_6oim_c1", "set_6oim_c8", "set_6oim_c64", "set_c21_c8", "set_6oim_c8_weights", "set_s64_c8", "set_l110_c8")


def qualifies(key, require, exclude) -> bool:
    have = {int(m) for m in key if int(m) != NONE}
    return all(have & {int(a) for a in g} for g in require) and not (have & {int(a) for a in exclude})


def constrained_first_max_key(leaves, C: int, require, exclude):
    """`first_max_key` over the leaves of `explain_ref.tree_leaves` whose key qualifies: (maxima [C], keys - None where no qualifying
    leaf scores > 0)."""
    return first_max_key([(key, sc) for key, sc in leaves if qualifies(key, require, exclude)], C)


def mask_clusters(words) -> list[int]:
    """The model clusters of a two-word bit mask (bit a % 64 of word a // 64)."""
    return [64 * w + b for w in range(2) for b in range(64) if (int(words[w]) >> b) & 1]


def load_constrained(name):
    """(model, library, weights, set npz, constrained fixture) of a golden set."""
    model, lib, weights, d = load_golden(name)
    return model, lib, weights, d, np.load(GOLDEN / f"constrained_{name}.npz")


def fixture_rows(x):
    """Per fixture row: (library index, kind, C, levels [nl], require groups, exclude list, scores [C], keys [C, nl] with -1 for None,
    gaps [C], unconstrained scores [C])."""
    for r, i in enumerate(x["index"]):
        C = int(x["n_conf"][r])
        lv = x["levels"][r]
        nl = int(np.count_nonzero(lv != 0xFE))
        key = x["key"][r, :C, :nl].astype(np.int64)
        key[key == 0xFF] = NONE
        require = [mask_clusters(x["require"][r, g]) for g in range(int(x["n_require"][r]))]
        yield (int(i), chr(int(x["kind"][r])), C, lv[:nl].astype(np.int64), require, mask_clusters(x["exclude"][r]), x["scores"][r, :C], key,
               x["gap"][r, :C], x["unconstrained"][r, :C])


def random_constraint(rng, clusters, K: int):
    """A seeded constraint over `clusters` (those worth asking for: the candidates of a ligand): one or two groups of 1 - 3 clusters,
    and - two times out of three - an exclude set of 1 - 2."""
    clusters = list(clusters) or list(range(K))
    groups = [sorted({int(a) for a in rng.choice(clusters, size=int(rng.integers(1, 4)))}) for _ in range(int(rng.integers(1, 3)))]
    exclude = sorted({int(a) for a in rng.choice(clusters, size=int(rng.integers(1, 3)))}) if rng.integers(0, 3) else []
    return groups, exclude


def walk_with_drops(model, record, weights7, require, exclude, tables=None):
    """The constrained walker's drop rule restated (csrc/pmx_explain.hip): the tree of `explain_ref.tree_leaves`, except that a child
    with >= 5 matches below which no leaf can qualify - an excluded cluster on its path, or a require group with no cluster on the path
    nor among the candidates of the levels below - is not walked and counts as one match; the skip child of a node with >= 5 matches
    likewise. Returns (maxima, keys, nodes walked): the maxima and keys must be those of the filtered full tree."""
    from explain_ref import Tables, candidates, ligand_levels

    T = tables or Tables(model, record, weights7)
    lv = ligand_levels(model, record)
    cand = [candidates(model, record, lc) for lc in lv]
    below = [set().union(*cand[l:]) if l < len(lv) else set() for l in range(len(lv) + 1)]  # candidates of level l and deeper
    require = [set(g) for g in require]
    exclude = set(exclude)
    C = T.C
    best = np.zeros(C)
    keys: list = [None] * C
    walked = [0]

    def feasible(have, more):
        return not (have & exclude) and all((have | more) & g for g in require)

    def dfs(level, path, scores):
        walked[0] += 1
        matched_here = bool(path) and path[-1][1] != NONE
        have = {m for _, m in path if m != NONE}
        if level == len(lv):
            if feasible(have, set()):
                for c, v in scores.items():
                    if v > best[c]:
                        best[c] = v
                        keys[c] = tuple(m for _, m in path)
            return int(matched_here)
        lc = lv[level]
        nm = sum(1 for _, m in path if m != NONE)  # (two levels may match one model cluster)
        mx = children = 0
        for mc in cand[level]:
            ok = {}
            for c, t in scores.items():
                acc, good = 0.0, True
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
                if nm + 1 >= 5 and not feasible(have | {mc}, below[level + 1]):
                    mx = max(mx, 1)
                    continue
                mx = max(mx, dfs(level + 1, path + [(lc, mc)], ok))
        if children == 0 or nm + mx < 5:
            if not (nm >= 5 and not feasible(have, below[level + 1])):
                mx = max(mx, dfs(level + 1, path + [(lc, NONE)], scores))
        return mx + int(matched_here)

    if lv and feasible(set(), below[0]):
        dfs(0, [], {c: 0.0 for c in range(C)})
    return best, keys, walked[0]
