"""NumPy / Python-int restatement of pmx_enrichment's specification (include/pmx.h) and of the host formulas on top of it.

Test infrastructure only: nothing in the package imports it. It shares no code with the package - the Poisson table is computed here
with `decimal`, the hash is written out again - so that agreement between the two means something."""

from __future__ import annotations

import math
from decimal import ROUND_FLOOR, Decimal, getcontext
from fractions import Fraction

import numpy as np

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def poisson1_table(digits: int = 80) -> list[int]:
    """T[m] = floor(2^64 * P(Poisson(1) <= m)) for m = 0 ... until it reaches 2^64 - 1 (that entry included)."""
    getcontext().prec = digits
    e = Decimal(1).exp()
    table, s = [], Fraction(0)
    for m in range(64):
        s += Fraction(1, math.factorial(m))
        table.append(int((Decimal(s.numerator) / Decimal(s.denominator) / e * Decimal(1 << 64)).to_integral_value(rounding=ROUND_FLOOR)))
        if table[-1] >= MASK:
            return table
    raise AssertionError("the table did not saturate")


TABLE = poisson1_table()
_TABLE_U64 = np.array(TABLE, dtype=np.uint64)


def mix_int(x: int) -> int:
    x &= MASK
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & MASK
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & MASK
    x ^= x >> 31
    return x


def count_int(seed: int, b: int, i: int) -> int:
    """c_i of row b, in Python integers (the slow, obviously right form)."""
    if b == 0:
        return 1
    h = mix_int(mix_int(seed + GOLDEN * b) + i)
    return sum(1 for t in TABLE if t <= h)


def _mix_u64(x: np.ndarray) -> np.ndarray:
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def counts(seed: int, b: int, n: int) -> np.ndarray:
    """int64 [n]: c_i of row b for ligands 0 .. n - 1."""
    if b == 0:
        return np.ones(n, dtype=np.int64)
    with np.errstate(over="ignore"):
        h = _mix_u64(np.uint64(mix_int(seed + GOLDEN * b)) + np.arange(n, dtype=np.uint64))
    return np.searchsorted(_TABLE_U64, h, side="right").astype(np.int64)


def canonical(scores, status=None) -> np.ndarray:
    """float64 [n]: the value a ligand is ranked by."""
    s = np.asarray(scores, dtype=np.float32).astype(np.float64)
    s = np.where(np.isnan(s), -np.inf, s)
    if status is not None:
        s = np.where(np.asarray(status) != 0, -np.inf, s)
    return s + 0.0  # (-0.0 + 0.0 is +0.0)


def ranked(scores, labels, status=None):
    """(order int64 [N'], head bool [N']): the counted ligands by descending value, ties by ascending index; head marks group starts."""
    key = canonical(scores, status)
    idx = np.flatnonzero(np.asarray(labels) < 2)
    order = idx[np.argsort(-key[idx], kind="stable")]
    k = key[order]
    head = np.ones(len(order), dtype=bool)
    head[1:] = k[1:] != k[:-1]
    return order.astype(np.int64), head


def cutoff_k(ppm: int, n_star: int) -> int:
    return (int(ppm) * int(n_star) + 999999) // 1000000


def walk(order, head, active, w, cut_ppm, alpha):
    """One (column, row): (u2 int, hits [n_cut] float64, expsum float). `active` bool [n], `w` int64 [n] by ligand index."""
    n_star = int(w[order].sum()) if len(order) else 0
    hits = np.zeros(len(cut_ppm), dtype=np.float64)
    if len(order) == 0:
        return 0, hits, 0.0
    starts = np.flatnonzero(head)
    wr = w[order]
    c_g = np.add.reduceat(wr, starts)
    a_g = np.add.reduceat(wr * active[order], starts)
    d_g = c_g - a_g
    c_after = np.cumsum(c_g)
    a_before = np.cumsum(a_g) - a_g
    c_before = c_after - c_g
    if 2 * int(a_g.sum()) * int(d_g.sum()) < 1 << 62:  # (no term and no partial sum can leave int64)
        u2 = int((d_g * (2 * a_before + a_g)).sum())
    else:
        u2 = sum(int(d) * (2 * int(ab) + int(a)) for d, ab, a in zip(d_g, a_before, a_g) if d)
    if n_star:
        for j, ppm in enumerate(cut_ppm):
            k = cutoff_k(ppm, n_star)
            g = int(np.searchsorted(c_after, k, side="left"))  # the first group that reaches k: it has c_g > 0 and C_before < k
            if k == int(c_after[g]):
                hits[j] = float(int(a_before[g]) + int(a_g[g]))
            else:
                hits[j] = float(int(a_before[g])) + float(int(a_g[g])) * float(k - int(c_before[g])) / float(int(c_g[g]))
    expsum = 0.0
    sel = a_g > 0
    if sel.any():
        s = -float(alpha) / float(n_star)
        cb, c, a = c_before[sel].astype(np.float64), c_g[sel].astype(np.float64), a_g[sel].astype(np.float64)
        terms = a * (np.exp(s * (cb + 1.0)) * np.expm1(s * c) * (1.0 / math.expm1(s)) / c)
        expsum = math.fsum(terms.tolist())
    return u2, hits, expsum


def enrichment_ref(scores, labels, status=None, cut_ppm=(5000, 10000, 50000), alpha=20.0, n_boot=0, seed=0):
    """The device outputs of pmx_enrichment as NumPy arrays: dict(totals, u2, hits, expsum, order). `scores` is [n] or [n_cols, n]."""
    scores = np.atleast_2d(np.asarray(scores, dtype=np.float32))
    labels = np.asarray(labels).astype(np.uint8)
    n_cols, n = scores.shape
    rows = 1 + n_boot
    counted = labels < 2
    active = labels == 1
    weights = [np.where(counted, counts(seed, b, n), 0) for b in range(rows)]
    totals = np.array([[int(w.sum()), int(w[active].sum()), int(w[counted & ~active].sum())] for w in weights], dtype=np.uint64).reshape(rows, 3)
    u2 = np.zeros((n_cols, rows), dtype=np.uint64)
    hits = np.zeros((n_cols, rows, len(cut_ppm)), dtype=np.float64)
    expsum = np.zeros((n_cols, rows), dtype=np.float64)
    orders = []
    for c in range(n_cols):
        order, head = ranked(scores[c], labels, status)
        orders.append(order)
        for b in range(rows):
            u, h, e = walk(order, head, active, weights[b], cut_ppm, alpha)
            u2[c, b], hits[c, b], expsum[c, b] = u, h, e
    return dict(totals=totals, u2=u2, hits=hits, expsum=expsum, order=np.stack(orders) if orders else np.zeros((0, 0), np.int64))


# ---------------------------------------------------------------------------------------------------------------- host formulas
def auroc(u2: int, n_a: int, n_d: int) -> float:
    return float("nan") if n_a == 0 or n_d == 0 else int(u2) / (2 * int(n_a) * int(n_d))


def ef(hits: float, ppm: int, n_star: int, n_a: int, n_d: int) -> float:
    if n_a == 0 or n_d == 0 or n_star == 0:
        return float("nan")
    return float(hits) * float(int(n_star)) / (float(cutoff_k(ppm, n_star)) * float(int(n_a)))  # (hits / k) / (n_a / N), with two roundings fewer


def bedroc(expsum: float, n_star: int, n_a: int, n_d: int, alpha: float) -> float:
    """Truchon & Bayly, J. Chem. Inf. Model. 2007, 47, 488: (RIE - RIE_min) / (RIE_max - RIE_min)."""
    if n_a == 0 or n_d == 0 or n_star == 0:
        return float("nan")
    n, ra = float(int(n_star)), int(n_a) / int(n_star)
    rie = (float(expsum) / int(n_a)) / ((1.0 / n) * (-math.expm1(-alpha)) / math.expm1(alpha / n))
    rie_max = -math.expm1(-alpha * ra) / (ra * -math.expm1(-alpha))
    rie_min = math.expm1(alpha * ra) / (ra * math.expm1(alpha))
    return (rie - rie_min) / (rie_max - rie_min)
