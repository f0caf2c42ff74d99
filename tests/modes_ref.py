"""Binding modes restated for the tests (`pmx_explain_modes`): per conformer the M best leaves of `explain_ref.tree_leaves` - those that
hold the conformer with a score > 0 and qualify under a constraint - by descending score, equal scores in iteration order; a CPU model
of the walker of csrc/pmx_explain.hip (M = 1: `pmx_explain`) with its drops; and the reading of tests/golden/modes_<set>.npz
(tests/golden/make_golden_modes.py)."""

from __future__ import annotations

import numpy as np

from conftest import GOLDEN, load_golden
from constrained_ref import CONSTRAINED_SETS, qualifies
from explain_ref import NONE, Tables, candidates, ligand_levels

MODES_SETS = CONSTRAINED_SETS
MAX_MODES = 8
SLACK = 1.0 + 1e-9  # kBoundSlack (csrc/pmx_screen_tables.h)


def ranked_modes(leaves, C: int, M: int, require=(), exclude=()):
    """(values [M, C], keys [M][C] - a tuple, or None past the list's end) of (key, {conformer: score}) leaves given in iteration order."""
    values = np.zeros((M, C))
    keys = [[None] * C for _ in range(M)]
    ok = [(tuple(key), sc) for key, sc in leaves if qualifies(key, require, exclude)]
    for c in range(C):
        have = [(sc[c], o) for o, (_, sc) in enumerate(ok) if sc.get(c, 0.0) > 0]
        have.sort(key=lambda e: (-e[0], e[1]))
        for m, (v, o) in enumerate(have[:M]):
            values[m, c] = v
            keys[m][c] = ok[o][0]
    return values, keys


def load_modes(name):
    """(model, library, weights, set npz, modes fixture) of a golden set."""
    model, lib, weights, d = load_golden(name)
    return model, lib, weights, d, np.load(GOLDEN / f"modes_{name}.npz")


def fixture_rows(x):
    """Per fixture ligand: (library index, C, levels [nl], values [8, C], keys [8, C, nl] with -1 for None, gaps [8, C], n_positive [C])."""
    for r, i in enumerate(x["index"]):
        C = int(x["n_conf"][r])
        lv = x["levels"][r]
        nl = int(np.count_nonzero(lv != 0xFE))
        key = x["key"][r, :, :C, :nl].astype(np.int64)
        key[key == 0xFF] = NONE
        yield int(i), C, lv[:nl].astype(np.int64), x["values"][r, :, :C], key, x["gap"][r, :, :C], x["n_positive"][r, :C]


def key_exact(gap, m: int, c: int) -> bool:
    """Is entry (m, c) of a fixture row pinned by key: its own gap and its predecessor's exceed 1e-5 (else by total)."""
    return gap[m, c] > 1e-5 and (m == 0 or gap[m - 1, c] > 1e-5)


def _walk(model, record, tables, leaf, drop=None):
    """The tree of `explain_ref.tree_leaves`, visited in iteration order. `leaf(path, scores, stack)`: stack[l] are the scores of the
    path's node at level l. `drop(level, path, scores)` is asked for a child with >= 5 matches and for the skip child of a node with
    >= 5 matches - the two sites at which the walker may leave a subtree out; a dropped child counts as one match. Returns nodes walked."""
    T = tables
    lv = ligand_levels(model, record)
    cand = [candidates(model, record, lc) for lc in lv]
    walked = [0]

    def dfs(level, path, stack):
        walked[0] += 1
        scores = stack[-1]
        matched_here = bool(path) and path[-1][1] != NONE
        if level == len(lv):
            leaf(path, scores, stack)
            return int(matched_here)
        lc = lv[level]
        nm = sum(1 for _, m in path if m != NONE)
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
                if nm + 1 >= 5 and drop is not None and drop(level + 1, path + [(lc, mc)], ok):
                    mx = max(mx, 1)
                    continue
                mx = max(mx, dfs(level + 1, path + [(lc, mc)], stack + [ok]))
        if children == 0 or nm + mx < 5:
            if not (nm >= 5 and drop is not None and drop(level + 1, path + [(lc, NONE)], scores)):
                mx = max(mx, dfs(level + 1, path + [(lc, NONE)], stack + [scores]))
        return mx + int(matched_here)

    if lv:
        dfs(0, [], [{c: 0.0 for c in range(T.C)}])
    return lv, cand, walked[0]


def completion_bounds(model, record, tables):
    """R [nl + 1, C]: the most any node of level l gains on its way to a leaf, per conformer - an admissible bound of what the levels from l
    on can add (the walker's own R is looser; any admissible bound must leave the answer alone)."""
    nl = len(ligand_levels(model, record))
    R = np.zeros((nl + 1, tables.C))

    def leaf(path, scores, stack):
        for l in range(nl + 1):
            for c, v in scores.items():
                R[l, c] = max(R[l, c], v - stack[l][c])

    _walk(model, record, tables, leaf)
    return R


def walk_modes_with_drops(model, record, weights7, M: int, require=(), exclude=(), tables=None, bounds=None):
    """The explain walker restated for M modes: per conformer M values, descending, and their keys; a leaf enters iff its total is strictly above the
    M-th value, behind every entry >= it; a subtree at a drop site is left out when no conformer it holds can reach its M-th value
    ((total + R) * slack < M-th, strictly) or - the constrained walker's rule - when no leaf below can qualify. Returns (values [M, C],
    keys [M][C], nodes walked): values and keys must be `ranked_modes` of the full tree."""
    T = tables or Tables(model, record, weights7)
    R = completion_bounds(model, record, T) if bounds is None else bounds
    lv = ligand_levels(model, record)
    cand = [candidates(model, record, lc) for lc in lv]
    below = [set().union(*cand[l:]) if l < len(lv) else set() for l in range(len(lv) + 1)]
    require = [set(g) for g in require]
    exclude = set(exclude)
    values = np.zeros((M, T.C))
    keys = [[None] * T.C for _ in range(M)]

    def feasible(have, more):
        return not (have & exclude) and all((have | more) & g for g in require)

    def leaf(path, scores, stack):
        if not feasible({m for _, m in path if m != NONE}, set()):
            return
        key = tuple(m for _, m in path)
        for c, t in scores.items():
            if t > values[M - 1, c]:
                at = M - 1
                while at > 0 and values[at - 1, c] < t:
                    values[at, c] = values[at - 1, c]
                    keys[at][c] = keys[at - 1][c]
                    at -= 1
                values[at, c] = t
                keys[at][c] = key

    def drop(level, path, scores):
        if not feasible({m for _, m in path if m != NONE}, below[level]):
            return True
        return not any((t + R[level, c]) * SLACK >= values[M - 1, c] for c, t in scores.items())

    walked = 0
    if feasible(set(), below[0]):
        _, _, walked = _walk(model, record, T, leaf, drop)
    return values, keys, walked
