"""`pmx_fingerprint_tanimoto` and `pmx_fingerprint_leaders` on the GPU (csrc/pmx_fingerprint.hip) against the NumPy rules of
tests/hotspot_ref.py: both are integer counts and one float32 division, so every comparison here is exact."""

from functools import lru_cache

import numpy as np
import pytest

from hotspot_ref import bits_to_words, leaders, tanimoto

pytestmark = pytest.mark.gpu


def fp_of(*nodes):
    bits = np.zeros(256, dtype=bool)
    bits[list(nodes)] = True
    return bits_to_words(bits)


def random_sets(rng, n, density=0.08):
    fp = bits_to_words(rng.random((n, 256)) < density)
    fp[rng.random(n) < 0.05] = 0  # some empty
    return fp


@lru_cache(maxsize=None)
def noisy_prototypes():
    """5000 fingerprints around 40 prototypes of about 20 bits, each bit of a copy flipped with probability 1 %; every tenth row an exact
    copy of its prototype (what threshold 1.0 joins). Made once, never written to."""
    rng = np.random.default_rng(7)
    proto = rng.random((40, 256)) < 0.08
    pick = rng.integers(0, 40, 5000)
    bits = proto[pick] ^ (rng.random((5000, 256)) < 0.01)
    bits[::10] = proto[pick[::10]]
    return bits_to_words(bits)


def test_tanimoto_matches_numpy():
    from pharmaconet_amd.engine import fingerprint_similarity

    rng = np.random.default_rng(3)
    a, b = random_sets(rng, 257), random_sets(rng, 130)
    a[0], b[0] = 0, 0  # empty against empty
    a[1], b[1] = fp_of(5, 70, 135, 200, 255), fp_of(200, 255)  # bits in word 3
    got = fingerprint_similarity(a, b)
    assert got.dtype == np.float32 and got.shape == (257, 130)
    assert np.array_equal(got.view(np.uint32), tanimoto(a, b).view(np.uint32))
    assert got[0, 0] == 1.0 and got[1, 1] == np.float32(2) / np.float32(5)
    one = fingerprint_similarity(a[:1], b)
    assert np.array_equal(one, got[:1])
    col = fingerprint_similarity(a, b[1:2])
    assert np.array_equal(col, got[:, 1:2])
    self_sim = fingerprint_similarity(a)  # a is b
    assert np.array_equal(self_sim.view(np.uint32), tanimoto(a, a).view(np.uint32))
    assert (np.diag(self_sim) == 1.0).all() and np.array_equal(self_sim, self_sim.T)
    assert fingerprint_similarity(a[:0], b).shape == (0, 130)


def test_leaders_hand_made_cases():
    from pharmaconet_amd.engine import fingerprint_leaders

    # a ~ b ~ c at 0.5 and a !~ c: c does not follow b into a's cluster
    chain = np.stack([fp_of(0, 1, 2, 3), fp_of(1, 2, 3, 4, 5), fp_of(2, 3, 4, 5, 6)])
    lead, of = fingerprint_leaders(chain, threshold=0.5)
    assert lead.tolist() == [0, 2] and of.tolist() == [0, 0, 2]
    rows = np.stack([fp_of(), fp_of(), fp_of(10), fp_of(10), fp_of(10, 250), fp_of(250)])
    lead, of = fingerprint_leaders(rows, threshold=1.0)
    assert lead.tolist() == [0, 2, 4, 5] and of.tolist() == [0, 0, 2, 2, 4, 5]
    rows = np.stack([fp_of(1), fp_of(2), fp_of(3), fp_of(2), fp_of(4), fp_of(1)])
    lead, of = fingerprint_leaders(rows, threshold=0.7, max_leaders=2)
    assert lead.tolist() == [0, 1] and of.tolist() == [0, 1, -1, 1, -1, 0]
    lead, of = fingerprint_leaders(rows, threshold=0.7, max_leaders=1)
    assert lead.tolist() == [0] and of.tolist() == [0, -1, -1, -1, -1, 0]
    lead, of = fingerprint_leaders(np.zeros((0, 4), dtype=np.uint64))
    assert len(lead) == 0 and len(of) == 0


@pytest.mark.parametrize("threshold", (0.5, 0.7, 1.0))
def test_leaders_of_noisy_prototypes(threshold):
    from pharmaconet_amd.engine import fingerprint_leaders

    fp = noisy_prototypes()
    for cap in (2048, 1):
        lead, of = fingerprint_leaders(fp, threshold=threshold, max_leaders=cap)
        ref_lead, ref_of = leaders(fp, threshold, cap)
        assert np.array_equal(lead, ref_lead) and np.array_equal(of, ref_of), (threshold, cap)
        assert len(ref_lead) == 1 if cap == 1 else len(ref_lead) >= 40


@pytest.mark.parametrize("n", (1, 63, 65, 1023, 1025, 4097))
def test_leaders_row_counts(n):
    """Row counts around the wavefront and the work-group, and every row its own leader until the leaders run out (4097 distinct rows,
    2048 leaders)."""
    from pharmaconet_amd.engine import fingerprint_leaders

    fp = noisy_prototypes()[:n]
    lead, of = fingerprint_leaders(fp, threshold=0.7)
    ref_lead, ref_of = leaders(fp, 0.7, 2048)
    assert np.array_equal(lead, ref_lead) and np.array_equal(of, ref_of)
    distinct = np.zeros((n, 4), dtype=np.uint64)
    distinct[:, 0] = np.arange(1, n + 1, dtype=np.uint64) << np.uint64(20)  # (rows that share at most half of their bits)
    distinct[:, 1] = ~(np.arange(1, n + 1, dtype=np.uint64) << np.uint64(20)) & np.uint64(0xFFFFF00000)
    lead, of = fingerprint_leaders(distinct, threshold=1.0)
    ref_lead, ref_of = leaders(distinct, 1.0, 2048)
    assert np.array_equal(lead, ref_lead) and np.array_equal(of, ref_of)
    assert len(lead) == min(n, 2048) and (of[2048:] == -1).all()


def test_leaders_refuses_what_the_header_rules_out():
    from pharmaconet_amd import _ffi
    from pharmaconet_amd.engine import fingerprint_leaders, fingerprint_similarity

    fp = noisy_prototypes()[:8]
    for kw in (dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=1.01), dict(threshold=float("nan")), dict(max_leaders=0), dict(max_leaders=2049)):
        with pytest.raises(_ffi.PmxError, match="libpmx error 1"):
            fingerprint_leaders(fp, **kw)
    with pytest.raises(ValueError):
        fingerprint_leaders(np.zeros((65537, 4), dtype=np.uint64))
    with pytest.raises(ValueError):
        fingerprint_similarity(np.zeros((65537, 4), dtype=np.uint64))
    lead, of = fingerprint_leaders(fp, threshold=0.7)  # (and the next call is served)
    assert lead[0] == 0 and of[0] == 0
