"""The specification of pmx_topk (include/pmx.h), restated once in NumPy, and the score families its tests rank.

The ranking step of screening.py:70 is `result.sort(key=score, reverse=True)`: a stable sort of a list in library order. pmx_topk adds
what a device buffer needs on top of it - NaN scores (unsupported ligands) after every real one, padding entries of a gathered list after
those - so the elements are ordered by (class, descending value, ascending position):

  class 0  a real score, +-inf included; values compare as IEEE floats, so -0.0 and +0.0 are one value
  class 1  NaN, any payload, either sign; among themselves in position order
  class 2  padding: indices[i] == -1 (UINT64_MAX), whatever its score; only when `indices` is given

The output is the first min(k, n) elements in that order, each score as given and each index `indices[pos]` or `base_index + pos`; the
tail up to k is -inf / -1. tests/test_topk_cpu.py pins this file to Python's own sort and to `distributed.merge_topk`.
"""

import numpy as np

FAMILIES = ("full", "ladder", "middle", "subnormal", "inf", "zeros", "nan")
NAN_BITS = (0x7FC00000, 0xFFC00001, 0x7F800001)  # quiet, negative quiet with a payload, signalling


def topk_ref(scores, k, base_index=0, indices=None):
    """(scores float32 [k], indices int64 [k], positions int64 [min(k, n)]) of the k best of `scores`."""
    s = np.ascontiguousarray(scores, dtype=np.float32).reshape(-1)
    n, k = s.size, int(k)
    cls = np.isnan(s).astype(np.int8)
    if indices is not None:
        idx = np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
        assert idx.size == n
        cls[idx == -1] = 2
    # (class, descending value) as one float64 that sorts ascending: a real score is -value, the infinities drawn in to -+1e300 (beyond
    # every finite float32, equal among themselves); every NaN is 2e300, every padding entry 4e300. -(-0.0) == -(+0.0).
    with np.errstate(invalid="ignore"):  # (the widening of a signalling NaN)
        key = np.where(cls == 0, np.clip(-s.astype(np.float64), -1e300, 1e300), cls * 2e300)
    # the sort is over the elements that can be among the first k alone: those not after the k-th smallest key (ties on it included)
    cand = np.flatnonzero(key <= np.partition(key, k - 1)[k - 1]) if 0 < k < n else np.arange(n)
    pos = cand[np.lexsort((key[cand],))[:k]]  # stable: equal keys stay in position order
    out_s = np.full(k, -np.inf, dtype=np.float32)
    out_i = np.full(k, -1, dtype=np.int64)
    out_s[: pos.size] = s[pos]
    out_i[: pos.size] = idx[pos] if indices is not None else np.int64(base_index) + pos
    return out_s, out_i, pos.astype(np.int64)


def same_scores(got, want):
    """Scores as given: a NaN where a NaN is wanted, every other score bit for bit (so -0.0 is not +0.0)."""
    got = np.ascontiguousarray(got, dtype=np.float32)
    want = np.ascontiguousarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def from_bits(bits):
    return np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32)


def gathered_lists(k=257, sizes=(400, 300, 500, 100), seed=0):
    """What `pmx_topk_allgather` merges, built by hand: every rank's k best of its contiguous shard (global indices; a shard shorter than
    k is padded with -inf / -1), concatenated in rank order. Few distinct scores, so ties run across ranks; -0.0 beside +0.0; NaNs.
    Returns (scores [ranks * k], indices [ranks * k], all shards' scores in library order)."""
    rng = np.random.default_rng([seed, k])
    values = np.array([1.25, 0.5, -0.0, 0.0, -0.5, np.nan, -np.inf], dtype=np.float32)
    share = (0.05, 0.05, 0.3, 0.3, 0.1, 0.1, 0.1)  # a tenth of the entries above the zeros: k = 257 of 1300 ends among the zeros
    shards = [values[rng.choice(len(values), size, p=share)] for size in sizes]
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    lists = [topk_ref(s, k, base_index=int(b))[:2] for s, b in zip(shards, first)]
    gs, gi = np.concatenate([l[0] for l in lists]), np.concatenate([l[1] for l in lists])
    assert (gi == -1).any() and np.isnan(gs).any() and {0x80000000, 0} <= set(gs.view(np.uint32).tolist())
    return gs, gi, np.concatenate(shards)


def score_family(name, n, seed=0):
    """float32 [n] of one family; the rank key of a score is a fold of its bits (csrc/pmx_device.h), selected in digits of 11 + 11 + 10 bits."""
    rng = np.random.default_rng([seed, FAMILIES.index(name), n])
    if name == "full":  # every digit of the key and both branches of the sign fold: random sign, exponent 0 .. 254, random mantissa
        bits = (rng.integers(0, 2, n, dtype=np.uint32) << 31) | (rng.integers(0, 255, n, dtype=np.uint32) << 23) | rng.integers(0, 1 << 23, n, dtype=np.uint32)
        return from_bits(bits)
    if name == "ladder":  # 4000 neighbours of 1.0 (1.0 and the 3999 floats above it): the keys agree in their top 20 bits
        return from_bits(np.uint32(0x3F800000) + rng.integers(0, 4000, n, dtype=np.uint32))
    if name == "middle":  # 1.0 + j 2^-13, j < 1500: the keys differ in bits 10 .. 20, the middle digit, only
        s = (1.0 + rng.integers(0, 1500, n) * 2.0**-13).astype(np.float32)
        assert np.all((s.view(np.uint32) & 0x3FF) == 0) and np.all(s.view(np.uint32) >> 21 == 0x3F800000 >> 21)
        return s
    if name == "subnormal":  # exponent 0: subnormals of both signs, one in five a zero of its sign
        mant = rng.integers(1, 1 << 23, n, dtype=np.uint32)
        mant[rng.random(n) < 0.2] = 0
        return from_bits((rng.integers(0, 2, n, dtype=np.uint32) << 31) | mant)
    if name == "inf":  # several copies of each infinity beside finite values
        s = rng.normal(0.0, 100.0, n).astype(np.float32)
        where = rng.choice(n, min(n, 14), replace=False)
        s[where[0::2]] = np.inf
        s[where[1::2]] = -np.inf
        return s
    if name == "zeros":  # 15 % -0.0, 15 % +0.0, 40 small positive values (so that a small k already cuts through the zeros), the rest negative
        s = -rng.integers(1, 50, n).astype(np.float32) * np.float32(0.125)
        u = rng.random(n)
        s[u < 0.15] = -0.0
        s[(u >= 0.15) & (u < 0.30)] = 0.0
        s[rng.choice(np.flatnonzero(u >= 0.30), min(40, n // 8), replace=False)] = rng.integers(1, 9, min(40, n // 8)).astype(np.float32) * np.float32(0.125)
        return s
    if name == "nan":  # 40 % NaN of three payloads and both signs among full-range scores
        s = score_family("full", n, seed + 1).copy()
        nan = rng.random(n) < 0.4
        s.view(np.uint32)[nan] = rng.choice(np.array(NAN_BITS, dtype=np.uint32), int(nan.sum()))
        return s
    raise KeyError(name)
