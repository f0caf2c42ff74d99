"""The ligand fingerprint's definition (`pmx_library_fingerprints`, include/pmx.h) on hand-made records whose bits are written out here:
what tests/ligand_fp_ref.py answers is what the GPU tests hold the kernel to, so the restatement is held to the header first. No GPU."""

import numpy as np
import pytest

import ligand_fp_ref as ref
from pharmaconet_amd.library import UNSUPPORTED_RECORD, PackedLibrary

HYD, ARO, CAT, ANI, DON, ACC, HAL = range(7)  # type ids (include/pmx.h PMX_NUM_TYPES)


def fingerprint(masks, positions, conformer=-1):
    """(set bits ascending, counts, status) of one hand-made record; `positions` [n, C, 3]."""
    lib = PackedLibrary.from_records([ref.make_record(masks, np.asarray(positions, dtype=np.float32).reshape(len(masks), -1, 3) if len(masks) else np.zeros((0, 1, 3), np.float32))])
    bits, counts, status = ref.record_fingerprint(lib.unpack(0), conformer)
    return np.flatnonzero(bits).tolist(), counts.tolist(), status


def two_nodes(x, ma=1 << HYD, mb=1 << HYD):
    return fingerprint([ma, mb], [[[0, 0, 0]], [[x, 0, 0]]])


def below(x):
    return float(np.nextafter(np.float32(x), np.float32(0)))


def test_bin_edges_are_closed_below():
    assert two_nodes(2.0)[0] == [1]  # d2 == 4: the edge belongs to the bin above it
    assert two_nodes(below(2.0))[0] == [0]
    assert two_nodes(12.0)[0] == [8]
    assert two_nodes(below(12.0))[0] == [7]
    assert two_nodes(0.0)[0] == [0] and two_nodes(1000.0)[0] == [8]
    for k, edge in enumerate((2.0, 3.0, 4.0, 5.0, 6.0, 7.5, 9.0, 12.0)):
        assert two_nodes(edge)[0] == [k + 1] and two_nodes(below(edge))[0] == [k]
    assert two_nodes(float("nan"))[0] == [0]  # a NaN reaches no edge


def test_squared_distance_is_float32_in_the_header_order():
    # dx = dy = 1 and dz = float32(sqrt 2): dz*dz rounds to 2 - 2^-23, and (1 + 1) + (2 - 2^-23) is a tie that float32 rounds to 4 - on the
    # edge, bin 1 - where the same sum in float64 stays below it
    z = np.float32(np.sqrt(np.float32(2.0)))
    assert np.float32(z * z) == np.float32(2.0) - np.float32(2.0**-23) and float(z) * float(z) + 2.0 < 4.0
    assert fingerprint([1, 1], [[[0, 0, 0]], [[1, 1, float(z)]]])[0] == [1]
    # 3-4-12: d2 = (9 + 16) + 144 = 169, and 2-3-6: 49, which is in [36, 56.25)
    assert fingerprint([1, 1], [[[0, 0, 0]], [[3, 4, 12]]])[0] == [8]
    assert fingerprint([1, 1], [[[1, 1, 1]], [[3, 4, 7]]])[0] == [5]


def test_type_pairs():
    seen = {ref.pair_index(a, b) for a in range(7) for b in range(a, 7)}
    assert seen == set(range(28))  # 28 distinct values below 28
    assert [ref.pair_index(0, b) for b in range(7)] == list(range(7)) and ref.pair_index(1, 1) == 7 and ref.pair_index(6, 6) == 27
    for a in range(7):
        for b in range(7):
            assert ref.pair_index(a, b) == ref.pair_index(b, a)
            got = two_nodes(3.5, 1 << a, 1 << b)
            assert got[0] == [ref.pair_index(a, b) * 9 + 2] and got == two_nodes(3.5, 1 << b, 1 << a)[:1] + got[1:]
    # both masks full: every one of the 28 type pairs, one bin each
    bits, counts, status = two_nodes(6.5, 0x7F, 0x7F)
    assert bits == [p * 9 + 5 for p in range(28)] and counts == [2] * 7 + [2] and status == 0
    assert max(bits) == 248 and two_nodes(20.0, 1 << HAL, 1 << HAL)[0] == [251]  # the last bit there is


def test_words_hold_bit_j_at_j_mod_64():
    bits = np.zeros(256, dtype=bool)
    bits[[0, 63, 64, 130, 251]] = True
    assert ref.bits_to_words(bits).tolist() == [1 | 1 << 63, 1, 1 << 2, 1 << 59]
    assert np.array_equal(ref.words_to_bits(ref.bits_to_words(bits))[0], bits)


def test_union_against_one_conformer():
    masks = [1 << ARO, 1 << ACC]
    pos = [[[0, 0, 0], [0, 0, 0]], [[2.5, 0, 0], [0, 8, 0]]]  # conformer 0: 2.5 A (bin 1), conformer 1: 8 A (bin 6)
    p = ref.pair_index(ARO, ACC)
    assert fingerprint(masks, pos)[0] == [p * 9 + 1, p * 9 + 6]
    assert fingerprint(masks, pos, 0)[0] == [p * 9 + 1] and fingerprint(masks, pos, 1)[0] == [p * 9 + 6]
    assert fingerprint(masks, pos, -1) == fingerprint(masks, pos)
    for bad in (2, -2, 64):
        bits, counts, status = fingerprint(masks, pos, bad)
        assert bits == [] and status == ref.KEY_INVALID and counts == [0, 1, 0, 0, 0, 1, 0, 2]  # the census is still written


def test_three_nodes_with_shared_types():
    masks = [1 << DON | 1 << ACC, 1 << CAT, 1 << DON]
    pos = [[[0, 0, 0]], [[3, 0, 0]], [[0, 4, 0]]]  # 3 A (bin 2), 4 A (bin 3), 5 A between the last two (bin 4)
    want = {ref.pair_index(DON, CAT) * 9 + 2, ref.pair_index(ACC, CAT) * 9 + 2, ref.pair_index(DON, DON) * 9 + 3, ref.pair_index(ACC, DON) * 9 + 3,
            ref.pair_index(CAT, DON) * 9 + 4}
    bits, counts, status = fingerprint(masks, pos)
    assert bits == sorted(want) and status == 0
    assert counts == [0, 0, 1, 0, 2, 1, 0, 3]


def test_empty_fingerprints():
    assert fingerprint([], np.zeros((0, 1, 3))) == ([], [0] * 8, 0)  # n = 0
    assert fingerprint([1 << ANI], [[[1, 2, 3]]]) == ([], [0, 0, 0, 1, 0, 0, 0, 1], 0)  # n = 1
    assert fingerprint([0, 1 << HYD], [[[0, 0, 0]], [[3, 0, 0]]]) == ([], [1, 0, 0, 0, 0, 0, 0, 2], 0)  # a mask of 0 pairs with nothing
    lib = PackedLibrary.from_records([UNSUPPORTED_RECORD])
    bits, counts, status = ref.record_fingerprint(lib.unpack(0))
    assert not bits.any() and not counts.any() and status == ref.UNSUPPORTED


def test_library_rows_and_search():
    records = [ref.make_record([1, 1], [[[0, 0, 0]], [[x, 0, 0]]]) for x in (1.0, 2.5, 3.5)] + [UNSUPPORTED_RECORD]
    lib = PackedLibrary.from_records(records)
    fp, tc, st = ref.library_fingerprints(lib)
    assert fp.tolist() == [[1, 0, 0, 0], [2, 0, 0, 0], [4, 0, 0, 0], [0, 0, 0, 0]] and st.tolist() == [0, 0, 0, 1] and tc[:, 7].tolist() == [2, 2, 2, 0]
    part = ref.library_fingerprints(lib, 1, 2)
    assert np.array_equal(part[0], fp[1:3]) and np.array_equal(part[1], tc[1:3])
    q = np.array([[3, 0, 0, 0], [0, 0, 0, 0]], dtype=np.uint64)
    out, fused = ref.search(q, fp)
    assert out.dtype == np.float32 and out.tolist() == [[0.5, 0.5, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]] and fused.tolist() == [0.5, 0.5, 0.0, 1.0]
    third = ref.search(np.array([[7, 0, 0, 0]], dtype=np.uint64), fp[:1])[0][0, 0]
    assert third == np.float32(1) / np.float32(3)
    lead, of = ref.leaders(np.array([[3, 0, 0, 0], [1, 0, 0, 0], [12, 0, 0, 0], [3, 0, 0, 0]], dtype=np.uint64), 0.5, 8)
    assert lead.tolist() == [0, 2] and of.tolist() == [0, 0, 2, 0]


@pytest.mark.parametrize("name", ("set_6oim_c8", "set_s64_c64"))
def test_fixtures_exercise_the_bit_range(name):
    from conftest import load_golden

    _, lib, _, _ = load_golden(name)
    fp, tc, st = ref.library_fingerprints(lib, 0, min(len(lib), 24))
    bits = ref.words_to_bits(fp)
    assert (st == 0).all() and not bits[:, 252:].any()
    assert bits.reshape(len(fp), -1)[:, :252].reshape(len(fp), 28, 9).any(axis=(0, 1)).all()  # all nine bins are populated
    assert len({f.tobytes() for f in fp}) >= len(fp) - 1 and 20 <= bits.sum(axis=1).mean() <= 90
    assert (tc[:, 7] == lib.headers()[: len(fp), 0]).all()
