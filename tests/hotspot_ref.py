"""A NumPy restatement of what `pmx_hotspots`, `pmx_fingerprint_tanimoto` and `pmx_fingerprint_leaders` answer, for the hotspot tests, on top
of tests/explain_ref.py's `Tables` and tests/attribution_ref.py's `attribution`: the same node pairs, per pair the inner terms g and
their 2-sigma test per model node pair (m, m'), and shares weighted by term * scale / G. float64 arithmetic, like the two it stands on."""

from __future__ import annotations

import itertools

import numpy as np

from attribution_ref import attribution
from explain_ref import NONE, Tables

WORDS = 4  # PMX_FINGERPRINT_WORDS


def inner_terms(T: Tables, a, b, c: int):
    """g [len(m1), len(m2)] and pass [len(m1), len(m2)] of the node pair (a, b) of `Tables._matches` lists for conformer c: the addends of
    `Tables._term`'s likelihood and its |z| < 2 test, one per model node pair."""
    (u, m1, w1), (v, m2, w2) = a, b
    d = float(T._dist(u, v)[c])
    mean = np.array([[T.flat.edge_mean[p, q] for q in m2] for p in m1], dtype=np.float64)
    std = np.array([[T.flat.edge_std[p, q] for q in m2] for p in m1], dtype=np.float64)
    z = (d - mean) / std
    return (w1[:, None] * w2[None, :]) / std * np.exp(-0.5 * z**2), np.abs(z) < 2.0


def bits_to_words(bits) -> np.ndarray:
    """bool [..., 256] -> uint64 [..., 4], bit m % 64 of word m // 64."""
    bits = np.asarray(bits, dtype=bool)
    full = np.zeros(bits.shape[:-1] + (64 * WORDS,), dtype=bool)
    full[..., : bits.shape[-1]] = bits
    return np.packbits(full, axis=-1, bitorder="little").view(np.uint64)


def words_to_bits(fp) -> np.ndarray:
    """uint64 [n, 4] -> bool [n, 256]."""
    fp = np.ascontiguousarray(np.asarray(fp, dtype=np.uint64).reshape(-1, WORDS))
    return np.unpackbits(fp.view(np.uint8), axis=1, bitorder="little").astype(bool)


def hotspots(model, rec, weights7, levels, key, c: int, tables: Tables | None = None) -> dict:
    """valid, total, share [Nm], terms [Nm], passes [Nm] and fingerprint (uint64 [4]) of the leaf `key` for conformer c. An invalid row has
    NaN total and shares and zero counts."""
    T = tables or Tables(model, rec, weights7)
    nm = T.flat.num_nodes
    at = attribution(model, rec, weights7, levels, key, c, T)
    share, terms, passes = np.zeros(nm), np.zeros(nm, dtype=np.int64), np.zeros(nm, dtype=np.int64)
    if not at["valid"]:
        return dict(valid=False, total=float("nan"), share=np.full(nm, np.nan), terms=terms, passes=passes, fingerprint=np.zeros(WORDS, dtype=np.uint64))
    nl = len(levels)
    key = [int(k) for k in key] + [NONE] * (nl - len(key))
    use = [l for l in range(nl) if key[l] != NONE]
    lists = {l: T._matches(int(levels[l]), key[l]) for l in use}
    entries = [((l, l), list(itertools.combinations(lists[l], 2))) for l in use]
    entries += [((l1, l2), list(itertools.product(lists[l1], lists[l2]))) for l1, l2 in itertools.combinations(use, 2)]
    for e, pairs in entries:
        term = [float(T._term(a, b)[0][c]) for a, b in pairs]
        acc = float(np.sum(term))
        scale = at["entry"][e] / acc if acc != 0.0 else 0.0
        for (a, b), t in zip(pairs, term):
            g, ok = inner_terms(T, a, b, c)
            G = float(g.sum())
            if G != 0.0:
                np.add.at(share, a[1], 0.5 * t * scale / G * g.sum(axis=1))
                np.add.at(share, b[1], 0.5 * t * scale / G * g.sum(axis=0))
            np.add.at(terms, a[1], g.shape[1])
            np.add.at(terms, b[1], g.shape[0])
            np.add.at(passes, a[1], ok.sum(axis=1))
            np.add.at(passes, b[1], ok.sum(axis=0))
    engaged = (terms > 0) & (2 * passes >= terms)
    return dict(valid=True, total=float(at["total"]), share=share, terms=terms, passes=passes, fingerprint=bits_to_words(engaged))


def matched_members(T: Tables, key) -> np.ndarray:
    """bool [Nm]: the model nodes that belong to a model cluster the key matches a level to."""
    out = np.zeros(T.flat.num_nodes, dtype=bool)
    for k in key:
        if int(k) != NONE:
            out[T.members[int(k)]] = True
    return out


def tanimoto(a, b) -> np.ndarray:
    """float32 [na, nb]: popcount(x & y) / popcount(x | y) as one float32 division, 1 where both are empty."""
    A, B = words_to_bits(a).astype(np.int64), words_to_bits(b).astype(np.int64)
    both = A @ B.T
    any_ = A.sum(axis=1)[:, None] + B.sum(axis=1)[None, :] - both
    with np.errstate(invalid="ignore", divide="ignore"):
        sim = both.astype(np.float32) / any_.astype(np.float32)
    return np.where(any_ == 0, np.float32(1.0), sim).astype(np.float32)


def leaders(fp, threshold: float, max_leaders: int):
    """The rule of `pmx_fingerprint_leaders`, row by row: (leaders, leader_of) with -1 for a row that joined none once `max_leaders` exist."""
    bits = words_to_bits(fp).astype(np.float32)  # (counts up to 256 are exact in float32)
    count = bits.sum(axis=1)
    thr = np.float32(threshold)
    held = np.zeros((max_leaders, bits.shape[1]), dtype=np.float32)  # the leaders' bits, in the order they were made
    held_count = np.zeros(max_leaders, dtype=np.float32)
    lead: list[int] = []
    leader_of = np.full(len(bits), -1, dtype=np.int64)
    for i in range(len(bits)):
        k = len(lead)
        if k:
            both = held[:k] @ bits[i]
            any_ = held_count[:k] + count[i] - both
            with np.errstate(invalid="ignore", divide="ignore"):
                sim = np.where(any_ == 0, np.float32(1.0), both / any_)
            hit = np.flatnonzero(sim >= thr)
            if len(hit):
                leader_of[i] = lead[int(hit[0])]
                continue
        if k < max_leaders:
            held[k], held_count[k] = bits[i], count[i]
            lead.append(i)
            leader_of[i] = i
    return np.asarray(lead, dtype=np.int64), leader_of
