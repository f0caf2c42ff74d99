"""The restatement of pmx_topk's specification (tests/topk_ref.py) held to the rule it restates - Python's stable descending sort,
screening.py:70 - and to the host merge `distributed.merge_topk`; and what `engine.topk` refuses before it hands addresses to the library."""

import time

import numpy as np
import pytest

import topk_ref as ref


def stable_desc(scores):
    values = scores.tolist()
    return sorted(range(len(values)), key=values.__getitem__, reverse=True)


@pytest.mark.parametrize("n", (5_003, 300_007))
@pytest.mark.parametrize("family", [f for f in ref.FAMILIES if f != "nan"])
def test_reference_is_pythons_stable_descending_sort(family, n):
    s = ref.score_family(family, n)
    assert not np.isnan(s).any()
    ranking = stable_desc(s)
    for k in (1, 64, 300, 4097, n, n + 3):
        got_s, got_i, pos = ref.topk_ref(s, k, base_index=1000)
        want = ranking[:k]
        assert pos.tolist() == want and got_i[: len(want)].tolist() == [1000 + p for p in want]
        assert ref.same_scores(got_s[: len(want)], s[want])
        assert np.all(got_i[len(want):] == -1) and np.all(np.isneginf(got_s[len(want):])) and len(got_s) == len(got_i) == k


def test_families_hold_what_they_are_for():
    zeros = ref.score_family("zeros", 5_003).view(np.uint32)
    assert (zeros == 0x80000000).sum() > 500 and (zeros == 0).sum() > 500
    sub = ref.score_family("subnormal", 5_003).view(np.uint32)
    assert np.all((sub >> 23) & 0xFF == 0) and (sub == 0x80000000).any() and (sub == 0).any() and ((sub & 0x7FFFFFFF) != 0).sum() > 3000
    assert len(np.unique(ref.score_family("ladder", 300_007))) == 4000 and len(np.unique(ref.score_family("middle", 300_007))) == 1500
    inf = ref.score_family("inf", 5_003)
    assert np.isposinf(inf).sum() == 7 and np.isneginf(inf).sum() == 7
    nan = ref.score_family("nan", 5_003)
    assert 0.35 < np.isnan(nan).mean() < 0.45 and set(nan.view(np.uint32)[np.isnan(nan)].tolist()) == set(ref.NAN_BITS)
    full = ref.score_family("full", 300_007).view(np.uint32)
    assert len(np.unique(full >> 21)) > 2000 and len(np.unique((full >> 10) & 0x7FF)) == 2048 and len(np.unique(full & 0x3FF)) == 1024


def test_signed_zeros_tie_in_index_order():
    s = np.array([-0.0, 0.0, -0.0, 0.0], dtype=np.float32)
    assert sorted(range(4), key=s.tolist().__getitem__, reverse=True) == [0, 1, 2, 3]
    got_s, got_i, _ = ref.topk_ref(s, 3)
    assert got_i.tolist() == [0, 1, 2] and got_s.view(np.uint32).tolist() == [0x80000000, 0, 0x80000000]  # reported as given


def test_classes_real_then_nan_then_padding():
    nan = ref.from_bits(ref.NAN_BITS)
    s = np.array([nan[0], -np.inf, 1e30, nan[1], 2.0, -np.inf, nan[2], np.inf], dtype=np.float32)
    i = np.array([10, 11, -1, 13, 14, -1, 16, 17], dtype=np.int64)
    got_s, got_i, pos = ref.topk_ref(s, 10, indices=i)
    assert pos.tolist() == [7, 4, 1, 0, 3, 6, 2, 5] and got_i.tolist() == [17, 14, 11, 10, 13, 16, -1, -1, -1, -1]
    assert ref.same_scores(got_s, np.concatenate([s[pos], np.full(2, -np.inf, dtype=np.float32)]))
    big = ref.topk_ref(s, 3, base_index=2**40 + 12_345)[1]
    assert big.tolist() == [2**40 + 12_345 + 7, 2**40 + 12_345 + 2, 2**40 + 12_345 + 4]  # (no indices: the 1e30 is a real score)


def test_reference_is_quick_at_the_largest_input():
    s = ref.score_family("full", 3 * 2**20 + 77)
    t0 = time.perf_counter()
    ref.topk_ref(s, 65_536)
    assert time.perf_counter() - t0 < 1.0


@pytest.mark.parametrize("k", (1, 100, 257, 700, 1028, 2000))
def test_host_merge_is_the_reference_on_gathered_lists(k):
    """`merge_topk` drops padding, so its list is the real part of the reference's: ties across ranks, -0.0 beside +0.0, NaNs."""
    from pharmaconet_amd.distributed import merge_topk

    gs, gi, everything = ref.gathered_lists()
    want_s, want_i, _ = ref.topk_ref(gs, k, indices=gi)
    real = want_i >= 0
    assert not real[int(real.sum()):].any()  # padding is last
    got_s, got_i = merge_topk(gs, gi, k)
    assert got_i.tolist() == want_i[real].tolist() and ref.same_scores(got_s, want_s[real])
    if k <= 257:  # every rank sent its k best, so the merge of the lists is the ranking of the whole library
        whole_s, whole_i, _ = ref.topk_ref(everything, k)
        assert whole_i.tolist() == want_i.tolist() and ref.same_scores(whole_s, want_s)


def test_engine_topk_refuses_what_it_would_misread(monkeypatch):
    import torch

    from pharmaconet_amd import _ffi, engine

    def no_library(*a, **kw):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_ffi, "load", no_library)
    s = torch.zeros(64, dtype=torch.float32)
    i = torch.arange(64, dtype=torch.int64)
    with pytest.raises(ValueError, match="float32"):
        engine.topk(s.double(), 4)
    with pytest.raises(ValueError, match="float32"):
        engine.topk(s.half(), 4)
    with pytest.raises(ValueError, match="not contiguous"):
        engine.topk(s[::2], 4)
    with pytest.raises(ValueError, match="on a GPU"):
        engine.topk(s, 4)
    with pytest.raises(ValueError, match="on a GPU"):
        engine.topk(s, 4, indices=i)
    with pytest.raises(ValueError, match="negative"):
        engine.topk(s, -1)
    with pytest.raises(ValueError, match="int64"):
        engine.topk(s, 4, indices=i.int())
    with pytest.raises(ValueError, match="int64"):
        engine.topk(s, 4, indices=i.double())
    with pytest.raises(ValueError, match="not contiguous"):
        engine.topk(s, 4, indices=torch.arange(128, dtype=torch.int64)[::2])
    with pytest.raises(ValueError, match="63 indices for 64 scores"):
        engine.topk(s, 4, indices=i[:63])
    with pytest.raises(ValueError, match="indices on meta"):
        engine.topk(s, 4, indices=torch.empty(64, dtype=torch.int64, device="meta"))
