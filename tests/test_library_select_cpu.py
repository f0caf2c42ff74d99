"""`PackedLibrary.select`: the host gather of records into a library of their own - the yardstick of the device gather
(`DeviceLibrary.select`, tests/test_gpu_library_select.py) - against `from_records` of the listed records, record by record."""

import numpy as np
import pytest

from conftest import load_golden

SETS = ("set_6oim_c8", "set_s64_c64")


@pytest.fixture(scope="module", params=SETS)
def lib(request):
    return load_golden(request.param)[1]


def same(a, b):
    return a.offsets.dtype == b.offsets.dtype and np.array_equal(a.offsets, b.offsets) and a.data.dtype == b.data.dtype and np.array_equal(a.data, b.data)


def by_records(lib, idx):
    from pharmaconet_amd import PackedLibrary

    return PackedLibrary.from_records([lib.record(int(i)) for i in idx])


def test_select_equals_the_listed_records(lib):
    n = len(lib)
    perm = np.random.default_rng(11).permutation(n)
    repeats = [0, n - 1, 0, 0, n // 2, n - 1, 1, n // 2]
    for idx in (perm, repeats, [], np.zeros(0, np.int64), [n - 1]):
        got = lib.select(idx)
        assert len(got) == len(idx) and same(got, by_records(lib, idx))
    assert lib.select([]).offsets.tolist() == [0] and lib.select([]).data.size == 0


def test_select_of_a_library_with_header_only_records(lib):
    from pharmaconet_amd import PackedLibrary
    from pharmaconet_amd.library import UNSUPPORTED_RECORD

    records = [lib.record(i) for i in range(min(len(lib), 6))]
    mixed = PackedLibrary.from_records([UNSUPPORTED_RECORD, records[0], UNSUPPORTED_RECORD, UNSUPPORTED_RECORD] + records[1:] + [UNSUPPORTED_RECORD])
    idx = np.random.default_rng(5).integers(0, len(mixed), 40)
    got = mixed.select(idx)
    assert same(got, by_records(mixed, idx))
    only = mixed.select([0, 2, 3, 0])
    assert only.data.tobytes() == UNSUPPORTED_RECORD * 4 and only.offsets.tolist() == [0, 16, 32, 48, 64]


def test_select_of_a_range_is_slice(lib):
    n = len(lib)
    for a, b in ((0, n), (1, n - 1), (n // 3, n // 3 + 4), (2, 2)):
        assert same(lib.select(range(a, b)), lib.slice(a, b - a))
        assert lib.select(range(a, b)).data.tobytes() == lib.slice(a, b - a).data.tobytes()


def test_select_refuses_an_index_outside_the_library(lib):
    n = len(lib)
    for idx in ([n], [0, 1, n + 5, 2], [-1], [0, -n - 1]):
        with pytest.raises(IndexError):
            lib.select(idx)
    with pytest.raises(IndexError, match="position 2"):
        lib.select([0, 1, n, n + 1])


def test_a_selection_survives_save_and_load(lib, tmp_path):
    from pharmaconet_amd import PackedLibrary

    idx = np.random.default_rng(3).permutation(len(lib))[: max(1, len(lib) // 2)]
    sel = lib.select(idx)
    sel.save(tmp_path / "sel.pmxlib")
    back = PackedLibrary.load(tmp_path / "sel.pmxlib")
    assert same(back, sel) and [back.record(i) for i in range(len(back))] == [lib.record(int(i)) for i in idx]
