"""pmx_topk (csrc/pmx_topk.hip) against the restatement of its specification (tests/topk_ref.py) wherever the radix select takes a
decision: every digit of the rank key (11 + 11 + 10 bits) and of the position (10 + 11 + 10 bits), both branches of the key's sign fold,
the infinities, subnormals, signed zeros and NaNs, k from 1 to 65536 beside n, the grid-stride loops, the `index_dev` path with padding,
the cached workspace and two streams. Every comparison is exact: indices as integers, scores bit for bit (a NaN for a NaN); there is no
tolerance anywhere in this file.

The tests that hold -0.0 beside +0.0 (the `zeros` and `subnormal` families, test_signed_zeros_*, test_three_merges_agree) fail on a
rank key that reads the zero's sign bit: -0.0 then ranks after every +0.0 instead of tying with it in index order."""

import ctypes
import functools

import numpy as np
import pytest

import topk_ref as ref

pytestmark = pytest.mark.gpu

N_BIG = 3 * 2**20 + 77  # above 2^21: the top digit of a position is not zero in the last third
KS = (1, 64, 300, 4097)


def rank(scores, k, base_index=0, indices=None):
    """engine.topk of host or device scores -> (scores, indices) on the host."""
    import torch

    from pharmaconet_amd.engine import topk

    t = scores if isinstance(scores, torch.Tensor) else torch.from_numpy(np.array(scores)).cuda()  # (a copy: `scores` may be read-only)
    ti = None if indices is None else torch.from_numpy(np.array(indices)).cuda()
    out_s, out_i = topk(t, k, base_index=base_index, indices=ti)
    return out_s.cpu().numpy(), out_i.cpu().numpy()


def expect(got, want, what="", scores_where=None):
    """Indices exactly and scores as given; `scores_where`: the ranks at which the scores are compared (all by default)."""
    (gs, gi), (ws, wi) = got, want[:2]
    assert gi.shape == wi.shape and gi.dtype == np.int64 and gs.dtype == np.float32
    bad = np.flatnonzero(gi != wi)
    assert bad.size == 0, f"{what}: {bad.size} of {wi.size} indices differ, the first at rank {bad[0]}: got {gi[bad[0]]}, want {wi[bad[0]]}"
    if scores_where is None:
        scores_where = np.ones(len(ws), dtype=bool)
    assert ref.same_scores(gs[scores_where], ws[scores_where]), f"{what}: scores differ"


@functools.lru_cache(maxsize=None)
def family(name, n):
    """(host scores, read-only; the same on the device) of one score family, made once."""
    import torch

    if name == "nan_heavy":  # 3000 real scores, every other one a NaN: the threshold of k = 4097 falls among the NaNs at any n
        s = ref.score_family("nan", n).copy()
        real = np.flatnonzero(~np.isnan(s))
        s.view(np.uint32)[real[3000:]] = np.resize(np.array(ref.NAN_BITS, dtype=np.uint32), max(0, real.size - 3000))
    elif name == "edges":  # full-range scores, one in a hundred a NaN
        s = ref.score_family("full", n, seed=7).copy()
        s.view(np.uint32)[np.random.default_rng(n).random(n) < 0.01] = ref.NAN_BITS[1]
    else:
        s = ref.score_family(name, n)
    t = torch.from_numpy(s).cuda()
    s.flags.writeable = False
    return s, t


# ------------------------------------------------------------------------------------------------------------------- score families
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", (5_003, 300_007))  # the second: every thread strides the grid more than once
@pytest.mark.parametrize("name", ref.FAMILIES + ("nan_heavy",))
def test_score_family(name, n, k):
    s, t = family(name, n)
    want = ref.topk_ref(s, k, base_index=1000)
    if name in ("nan", "nan_heavy") and k > (~np.isnan(s)).sum():  # winners past the real scores: the NaNs in position order, each with its index
        real = int((~np.isnan(s)).sum())
        assert np.isnan(want[0][real:]).all() and (np.diff(want[2][real:]) > 0).all() and len(set(s.view(np.uint32)[want[2][real:]].tolist())) == 3
    expect(rank(t, k, base_index=1000), want, f"{name}, n = {n}, k = {k}")


def test_nan_threshold_is_reached():
    """The cases above in which k exceeds the count of real scores exist: the threshold of the select falls inside the NaN group."""
    for name, n in (("nan", 5_003), ("nan_heavy", 5_003), ("nan_heavy", 300_007)):
        s = family(name, n)[0]
        assert (~np.isnan(s)).sum() < 4097 < n


@pytest.mark.parametrize("n", (5_003, 300_007))
def test_signed_zeros_cut_by_k(n):
    """-0.0 and +0.0 are one value: they tie in index order, and a k that ends among them takes the first of them, of either sign, each
    reported with the sign it has."""
    s, t = family("zeros", n)
    bits = s.view(np.uint32)
    neg, pos, above = int((bits == 0x80000000).sum()), int((bits == 0).sum()), int((s > 0).sum())
    assert neg > 0.1 * n and pos > 0.1 * n and above == 40
    for k in (above + 1, above + 2, 64, 300, above + (neg + pos) // 2, above + neg + pos - 1):
        if k > 65_536:
            continue
        want = ref.topk_ref(s, k)
        taken = s.view(np.uint32)[want[2][above:]]
        assert np.all(s[want[2][above:]] == 0) and (np.diff(want[2][above:]) > 0).all()  # k cuts through the zeros, which go by position
        if k >= 64:
            assert (taken == 0x80000000).any() and (taken == 0).any()
        expect(rank(t, k), want, f"zeros, n = {n}, k = {k}")


def test_signed_zeros_smallest_case():
    s = np.array([-0.0, 0.0, -0.0, 0.0], dtype=np.float32)
    for k in (1, 2, 3, 4, 6):
        got = rank(s, k)
        assert got[1].tolist() == [0, 1, 2, 3, -1, -1][:k]
        expect(got, ref.topk_ref(s, k), f"four zeros, k = {k}")
    assert rank(s, 3)[0].view(np.uint32).tolist() == [0x80000000, 0, 0x80000000]  # a winning -0.0 is reported as -0.0


# ----------------------------------------------------------------------------------------------------------------- position digits
@functools.lru_cache(maxsize=None)
def background():
    s = np.random.default_rng(11).random(N_BIG, dtype=np.float32) * np.float32(0.5)  # strictly below the tie value 1.0
    s.flags.writeable = False
    return s


ABOVE = np.array([7, 12_345, 2**20 + 1, 2**21 + 17, N_BIG - 1])


def tied_at(positions):
    """Background scores below 1.0, five scores above it, and 1.0 at `positions`: (host, device)."""
    import torch

    assert not np.isin(ABOVE, positions).any() and len(np.unique(positions)) == len(positions) and positions.max() < N_BIG
    s = background().copy()
    s[positions] = 1.0
    s[ABOVE] = (2.0, 3.0, 4.0, 5.0, 6.0)
    return s, torch.from_numpy(s).cuda()


def check_ties(scores, positions, taken):
    """k = the five above and the first `taken` ties: the last winner is the tie at sorted(positions)[taken - 1]."""
    s, t = scores
    k = len(ABOVE) + taken
    want = ref.topk_ref(s, k, base_index=5)
    positions = np.sort(positions)
    assert want[2][len(ABOVE):].tolist() == positions[:taken].tolist() and taken < len(positions)
    expect(rank(t, k, base_index=5), want, f"{len(positions)} ties, k = {k}")
    return int(want[2][-1])


def test_ties_spread_over_the_whole_array():
    """A tie about every 40 000th position; the last one taken lies in the final third, past 2^21: all three position digits decide."""
    rng = np.random.default_rng(5)
    positions = np.arange(1000, N_BIG - 1000, 40_000) + rng.integers(0, 1000, len(np.arange(1000, N_BIG - 1000, 40_000)))
    last = check_ties(tied_at(positions), positions, 61)
    assert last > 2**21 and last > 2 * N_BIG // 3 and (np.sort(positions)[61:] > last).all()


def test_ties_in_one_run_past_2_21():
    """600 ties in a row from 2^21 + 3 * 2^10 + 5, k ending inside the run: the low position digit alone varies (and its carry)."""
    positions = 2**21 + 3 * 2**10 + 5 + np.arange(600)
    scores = tied_at(positions)
    assert check_ties(scores, positions, 300) == 2**21 + 3 * 2**10 + 5 + 299
    check_ties(scores, positions, 1)
    check_ties(scores, positions, 599)


def test_ties_one_per_low_digit_block():
    """Ties at j * 2^10 + 7 for 3000 consecutive j: the low digit is constant, the middle one varies, the top one changes on the way."""
    positions = np.arange(50, 3050) * 2**10 + 7
    scores = tied_at(positions)
    assert check_ties(scores, positions, 2500) == (50 + 2499) * 2**10 + 7 > 2**21
    check_ties(scores, positions, 1998)  # the last winner just below 2^21 ...
    check_ties(scores, positions, 1999)  # ... and the first tie at or above it: (50 + 1998) * 2^10 = 2^21


def test_all_scores_equal():
    import torch

    t = torch.full((N_BIG,), 0.25, dtype=torch.float32, device="cuda")
    got_s, got_i = rank(t, 65_536)
    assert np.array_equal(got_i, np.arange(65_536)) and np.all(got_s == np.float32(0.25))


# -------------------------------------------------------------------------------------------------------------------- k and n edges
EDGE_KS = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 32_769, 65_535, 65_536)


@pytest.mark.parametrize("k,n", [(k, n) for k in EDGE_KS for n in (k - 1, k, k + 1, 300_007) if n > 0])
def test_k_beside_n_and_powers_of_two(k, n):
    s, t = family("edges", n)
    expect(rank(t, k, base_index=3), ref.topk_ref(s, k, base_index=3), f"n = {n}, k = {k}")


def test_no_scores_at_all():
    got_s, got_i = rank(np.zeros(0, dtype=np.float32), 5)
    assert got_i.tolist() == [-1] * 5 and np.isneginf(got_s).all()


@pytest.mark.parametrize("n", (1, 255, 256, 257, 1023, 1024, 1025, 1024 * 1024 + 1))
def test_n_beside_block_and_grid_sizes(n):
    s, t = family("edges", n)
    expect(rank(t, 17), ref.topk_ref(s, 17), f"n = {n}, k = 17")


def test_c_abi_k_zero_and_refusals():
    """k = 0 is served and writes nothing; k above 65536, a negative k and n = 2^31 are refused before anything is launched (one score
    is enough behind the pointer); the call after each is served."""
    import torch

    from pharmaconet_amd import _ffi

    lib = _ffi.load()
    s, t = family("full", 5_003)
    one = torch.zeros(1, dtype=torch.float32, device="cuda")
    out_s = torch.empty(8, dtype=torch.float32, device="cuda")
    out_i = torch.empty(8, dtype=torch.int64, device="cuda")
    device = torch.cuda.current_device()

    def poison():
        out_s.fill_(123.0)
        out_i.fill_(77)

    def untouched():
        torch.cuda.synchronize()
        return out_s.cpu().tolist() == [123.0] * 8 and out_i.cpu().tolist() == [77] * 8

    def call(scores, n, k):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        return lib.pmx_topk(scores.data_ptr(), None, n, 0, k, out_s.data_ptr(), out_i.data_ptr(), device, stream)

    def served():
        assert call(t, 5_003, 8) == 0
        torch.cuda.synchronize()
        expect((out_s.cpu().numpy(), out_i.cpu().numpy()), ref.topk_ref(s, 8), "the call after")
        poison()

    poison()
    assert call(t, 5_003, 0) == 0 and untouched()
    served()
    for scores, n, k, message in ((t, 5_003, 65_537, b"65536"), (t, 5_003, -1, b"argument"), (one, 2**31, 8, b"2^31")):
        assert call(scores, n, k) != 0
        assert message in lib.pmx_last_error()
        assert untouched()
        served()


# ------------------------------------------------------------------------------------------------------------------ index_dev path
def ascending_indices(n, seed=1):
    return 2**40 + np.cumsum(np.random.default_rng(seed).integers(1, 1000, n)).astype(np.int64)


def test_64_bit_indices():
    s, t = family("full", 300_007)
    idx = ascending_indices(len(s))
    assert idx[0] > 2**40 and idx[-1] - idx[0] > 2**26
    expect(rank(s, 300, indices=idx), ref.topk_ref(s, 300, indices=idx), "indices above 2^40")
    expect(rank(t, 300, base_index=2**40 + 12_345), ref.topk_ref(s, 300, base_index=2**40 + 12_345), "base_index above 2^40")


@pytest.mark.parametrize("padding_score", (-np.inf, 1e30))
def test_padding_interleaved(padding_score):
    """Padding entries (index -1) anywhere in the list rank after every NaN, whatever their score; where k exceeds the real scores and
    the NaNs (and n exceeds k) the threshold falls inside the padding group and the padding taken reads index -1."""
    n = 5_003
    rng = np.random.default_rng(21)
    s = ref.score_family("full", n, seed=3).copy()
    u = rng.random(n)
    s.view(np.uint32)[u < 0.05] = rng.choice(np.array(ref.NAN_BITS, dtype=np.uint32), int((u < 0.05).sum()))
    s[rng.choice(np.flatnonzero(u >= 0.3), 10, replace=False)] = -np.inf  # real scores of -inf: before every NaN
    idx = ascending_indices(n)
    pad = (u >= 0.05) & (u < 0.27)
    s[pad] = padding_score
    idx[pad] = -1
    real, nans = int((~pad & ~np.isnan(s)).sum()), int(np.isnan(s).sum())
    assert real + nans + 60 < 4097 < n and pad[:50].any() and pad[-50:].any() and not pad[-50:].all()
    for k in (300, real - 3, real + 7, real + nans, real + nans + 1, real + nans + 50, 4097, n - 1, n, n + 5):
        want = ref.topk_ref(s, k, indices=idx)
        assert np.all(want[1][real + nans : min(k, n)] == -1) and np.all(want[1][: min(k, real + nans)] >= 2**40)
        expect(rank(s, k, indices=idx), want, f"padding {padding_score}, k = {k}", scores_where=want[1] != -1 if padding_score > 0 else None)


def test_three_merges_agree():
    """One gathered buffer (4 ranks x k = 257; ties across ranks, -0.0 beside +0.0, NaNs, a short last shard) merged by the host
    (`merge_topk`), by the restatement and by the device - what `pmx_topk_allgather` runs behind its all-gather."""
    from pharmaconet_amd.distributed import merge_topk

    gs, gi, everything = ref.gathered_lists()
    for k in (257, 100, 1028):
        want = ref.topk_ref(gs, k, indices=gi)
        got = rank(gs, k, indices=gi)
        expect(got, want, f"gathered lists, k = {k}")
        host_s, host_i = merge_topk(gs, gi, k)
        assert host_i.tolist() == got[1][: len(host_i)].tolist() and ref.same_scores(host_s, got[0][: len(host_i)]) and np.all(got[1][len(host_i):] == -1)
    expect(rank(gs, 257, indices=gi), ref.topk_ref(everything, 257), "the merge of the lists is the ranking of the library")


# ----------------------------------------------------------------------------------------------------------- workspace and streams
def test_workspace_is_reused_across_k():
    """One stream, k = 65536, then 3, then 65536 again over other inputs: the cached workspace holds the larger call's candidates."""
    a, b, c = family("full", 300_007), family("ladder", 300_007), family("edges", 300_007)
    for (s, t), k in ((a, 65_536), (b, 3), (c, 65_536), (b, 1), (a, 4097)):
        expect(rank(t, k), ref.topk_ref(s, k), f"k = {k} after another k")


def test_two_streams():
    """One input ranked on two streams, enqueued alternately (each stream has a workspace of its own), read after each is synchronised."""
    import torch

    from pharmaconet_amd.engine import topk

    s, t = family("ladder", 300_007)
    torch.cuda.synchronize()
    streams = (torch.cuda.Stream(), torch.cuda.Stream())
    ks = (300, 4097)
    results = ([], [])
    for _ in range(3):
        for which in (0, 1):
            with torch.cuda.stream(streams[which]):
                results[which].append(topk(t, ks[which], base_index=which))
    for which in (0, 1):
        streams[which].synchronize()
        want = ref.topk_ref(s, ks[which], base_index=which)
        for out_s, out_i in results[which]:
            expect((out_s.cpu().numpy(), out_i.cpu().numpy()), want, f"stream {which}")
    torch.cuda.synchronize()


def test_repeats_are_bit_identical():
    """The compaction fills its slots in the order of an atomic counter; the sort of the winners hides that order."""
    s, t = family("ladder", 300_007)
    first = rank(t, 4097)
    expect(first, ref.topk_ref(s, 4097), "first call")
    for _ in range(2):
        again = rank(t, 4097)
        assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
