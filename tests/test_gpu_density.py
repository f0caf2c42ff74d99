"""`csrc/pmx_density.hip` through the C ABI (`pmx_density_create / _labels / _order / _destroy`) against the plain restatement
(tests/density_ref.py, pinned on the CPU by tests/test_density_cpu.py), the seeds chosen here and not by CPython's `set.pop()`:
component labels at every grid size from one voxel to 128^3 and on paths that need thousands of sweeps; member order at frontier
widths beside a wavefront, a workgroup and the scan's chunk sizes, over thousands of levels, and for hundreds of components in one
call; repeated, partial, short and long slices; the refusals; the special float values; and the Python wrapper around the calls.
Every comparison is exact, on integers."""

import contextlib
import ctypes
import functools

import numpy as np
import pytest

import density_ref as ref

pytestmark = pytest.mark.gpu

POISON = -7  # what the members buffer holds before a call: the calls write members or -1


def libpmx():
    from pharmaconet_amd import _ffi

    return _ffi.load()


def i32(values):
    return np.ascontiguousarray(np.asarray(values, dtype=np.int32))


@contextlib.contextmanager
def density(maps):
    """The handle of pmx_density_create over `maps` (a list of [S, S, S] maps or a [n, S, S, S] stack)."""
    lib = libpmx()
    stack = np.ascontiguousarray(np.stack([np.asarray(m, dtype=np.float32) for m in maps]))
    assert stack.ndim == 4 and stack.shape[1] == stack.shape[2] == stack.shape[3]
    handle = ctypes.c_void_p()
    rc = lib.pmx_density_create(stack.ctypes.data, stack.shape[0], stack.shape[1], 0, ctypes.byref(handle))
    assert rc == 0, lib.pmx_last_error()
    try:
        yield handle
    finally:
        lib.pmx_density_destroy(handle)


def device_labels(handle, n_maps, size):
    out = np.full(n_maps * size**3, POISON, dtype=np.int32)
    assert libpmx().pmx_density_labels(handle, out.ctypes.data) == 0
    return out.reshape(n_maps, size**3)


def device_order(handle, comps, offsets=None, status=0):
    """pmx_density_order for comps = [(map, seed, slice length)]: the slices as lists (None where the call is refused)."""
    lib = libpmx()
    if offsets is None:
        offsets = np.concatenate([[0], np.cumsum([c[2] for c in comps])])
    offsets = i32(offsets)
    cm, cs = i32([c[0] for c in comps]), i32([c[1] for c in comps])
    members = np.full(max(int(offsets.max(initial=0)), 1) + 8, POISON, dtype=np.int32)
    rc = lib.pmx_density_order(handle, len(comps), cm.ctypes.data, cs.ctypes.data, offsets.ctypes.data, members.ctypes.data)
    assert rc == status, (rc, lib.pmx_last_error())
    if status != 0:
        assert b"pmx_density_order" in lib.pmx_last_error()
        assert (members == POISON).all()
        return None
    total = int(offsets[len(comps)]) if len(comps) else 0
    assert (members[total:] == POISON).all()  # nothing is written behind the last slice
    return [members[offsets[c]:offsets[c + 1]].tolist() for c in range(len(comps))]


# ------------------------------------------------------------------------------------------------------------------------- labels
def sparse_128():
    """Three blobs, the eight corners and voxels on each face of a 128^3 map."""
    size = 128
    rng = np.random.default_rng(128)
    m = np.zeros((size, size, size), dtype=np.float32)
    for c, r in (((20, 30, 40), 5.5), ((64, 64, 64), 4.2), ((120, 100, 9), 6.0)):
        g = np.stack(np.meshgrid(*[np.arange(-7, 8)] * 3, indexing="ij"), -1)
        for d in g[(g**2).sum(-1) <= r * r]:
            m[tuple(np.asarray(c) + d)] = rng.uniform(0.05, 1.0)
    for corner in np.ndindex(2, 2, 2):
        m[tuple(127 * np.asarray(corner))] = 0.4
    for axis in range(3):
        for side in (0, 127):
            for _ in range(3):
                p = rng.integers(1, 127, size=3)
                p[axis] = side
                m[tuple(p)] = m[tuple(np.clip(p + (0, 1, 1), 0, 127))] = rng.uniform(0.05, 1.0)
    return m


def label_maps(size):
    rng = np.random.default_rng(9000 + size)
    if size == 128:
        return [sparse_128()]
    maps = [ref.blobs(size, max(2, size // 3), rng, speck=0.003 if size >= 16 else 0.0) for _ in range(2)]
    for density_of_voxels in (0.3, 0.08):  # one sprawling component that takes many sweeps; many small ones of every shape
        maps.append((rng.uniform(0.05, 1.0, size=(size,) * 3) * (rng.random((size,) * 3) < density_of_voxels)).astype(np.float32))
        if size >= 64:
            maps[-1][8:] = 0  # (the restatement is a Python loop: keep the random voxels to eight planes)
    if size >= 4:
        maps.append(ref.wrap_traps(size))
    maps.append(np.zeros((size,) * 3, dtype=np.float32))
    if size <= 16:
        maps.append(ref.full(size))
    one = np.zeros((size,) * 3, dtype=np.float32)
    one[-1, -1, -1] = 0.5
    maps.append(one)
    return maps


@pytest.mark.parametrize("size", (1, 2, 3, 5, 8, 11, 16, 32, 64, 128))
def test_labels_at_every_size(size):
    """S <= 10: fewer voxels than the label kernel has threads; 11: the first size above that; 128: 2048 voxels per thread in the
    start-up loop. Every voxel of every map, the -1s included."""
    maps = label_maps(size)
    with density(maps) as handle:
        got = device_labels(handle, len(maps), size)
    for k, m in enumerate(maps):
        want = ref.labels_ref(m)
        bad = np.flatnonzero(got[k] != want)
        assert bad.size == 0, f"S = {size}, map {k}: {bad.size} labels differ, the first at {bad[0]}: got {got[k][bad[0]]}, want {want[bad[0]]}"


@pytest.mark.parametrize("size", (16, 32))
def test_label_convergence_on_the_snakes(size):
    """One component that is a single path of 1087 / 8447 voxels, as built, flipped and permuted: the smallest index has to travel
    the whole path, with and against the order of the sweep."""
    variants = ref.snake_variants(size)
    with density(list(variants.values())) as handle:
        got = device_labels(handle, len(variants), size)
    for k, (name, m) in enumerate(variants.items()):
        on = m.reshape(-1) > 0
        assert len(np.unique(got[k][on])) == 1, f"{name}: {len(np.unique(got[k][on]))} labels on one component"
        assert np.array_equal(got[k], ref.labels_ref(m)), name


def test_maps_next_to_each_other_are_independent():
    stack = ref.wrap_trap_stack(4, 3)
    with density(stack) as handle:
        got = device_labels(handle, 3, 4)
        lists = device_order(handle, [(m, v, 1) for m in range(3) for v in (0, 63)])
    for k in range(3):
        assert got[k].tolist() == [0] + [-1] * 62 + [63]
    assert lists == [[0], [63]] * 3


def float_map():
    tiny, sub = np.finfo(np.float32).tiny, np.float32(1e-45)
    assert 0 < sub < tiny and sub.view(np.uint32) == 1
    m = np.zeros((8, 8, 8), dtype=np.float32)
    specials = (np.float32(-0.0), np.float32(-2.5), np.float32(np.nan), np.float32(np.inf), sub, tiny, np.float32(0.75))
    places = ((0, 0), (0, 3), (0, 6), (3, 0), (3, 3), (3, 6), (6, 0))
    for (x, y), v in zip(places, specials):
        m[x, y, 1:4] = (0.5, v, 0.25)  # a row that is one component only if v counts as active
    m[6, 4, 4], m[7, 5, 5], m[6, 6, 6] = 0.5, sub, 0.5  # joined through a corner by a subnormal
    return m, places


def test_float_values():
    """Active is what `mask > 0` says in NumPy float32: the subnormal, FLT_MIN and +inf are, -0.0, a negative value and NaN are not."""
    m, places = float_map()
    want = ref.labels_ref(m)
    comps = ref.components(m)
    assert len(comps) == 3 * 2 + 4 + 1 and sorted(len(c) for c in comps.values()) == [1] * 6 + [3] * 5
    with density([m]) as handle:
        got = device_labels(handle, 1, 8)[0]
        for (x, y), joined in zip(places, (False, False, False, True, True, True, True)):
            row = got[[ref.linear((x, y, z), 8) for z in (1, 2, 3)]].tolist()
            first = ref.linear((x, y, 1), 8)
            assert row == ([first] * 3 if joined else [first, -1, first + 2]), (x, y, row)
        assert np.array_equal(got, want)
        for pick in (min, max):
            asked = [(0, int(pick(c)), len(c)) for c in comps.values()]
            assert device_order(handle, asked) == [ref.bfs_order(m, seed) for _, seed, _ in asked]


# -------------------------------------------------------------------------------------------------------------------------- order
@pytest.mark.parametrize("n", (63, 64, 65, 255, 256, 257, 511, 512, 513))
def test_order_of_a_prism(n):
    """Levels of exactly n voxels (tests/test_density_cpu.py counts them): one wavefront and one voxel either side, one workgroup
    of the order kernel, and two voxels per thread of its scan going on three. From a corner, then from the middle: two fronts."""
    m = ref.prism(32, n)
    cells = np.argwhere(m[16] > 0)
    middle = (16, *cells[len(cells) // 2].tolist())
    with density([m]) as handle:
        for seed in ((0, 0, 0), middle):
            want = ref.bfs_order(m, seed)
            assert len(want) == 32 * n
            got = device_order(handle, [(0, ref.linear(seed, 32), 32 * n)])[0]
            bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
            assert bad.size == 0, f"prism {n} from {seed}: {bad.size} members differ, the first at {bad[0]}"


def test_order_of_a_full_grid():
    m = ref.full(32)
    with density([m]) as handle:
        got = device_order(handle, [(0, ref.linear((5, 7, 11), 32), 32768)])[0]
    assert got == ref.bfs_order(m, (5, 7, 11))


def test_order_of_the_smallest_full_grids():
    with density([ref.full(3)]) as handle:
        assert device_order(handle, [(0, 13, 27)])[0] == [13] + [v for v in range(27) if v != 13]
    with density([ref.full(2)]) as handle:
        assert device_order(handle, [(0, 0, 8)])[0] == list(range(8))
    with density([ref.full(1)]) as handle:
        assert device_order(handle, [(0, 0, 1)])[0] == [0]


@pytest.mark.parametrize("size", (16, 32))
def test_order_along_the_snakes(size):
    """Thousands of levels of one or two voxels: from an end, and from a voxel in the middle (two arms, levels of up to four)."""
    m = ref.snake(size)
    path = ref.snake_path(size)
    with density([m]) as handle:
        for seed in (path[0], path[-1], path[len(path) // 2]):
            want = ref.bfs_order(m, seed)
            assert len(want) == len(path)
            assert device_order(handle, [(0, ref.linear(seed, size), len(path))])[0] == want, seed


def test_order_of_512_single_voxels():
    m = ref.lattice(16)
    seeds = np.flatnonzero(m.reshape(-1) > 0).tolist()
    assert len(seeds) == 512
    with density([m]) as handle:
        assert device_order(handle, [(0, v, 1) for v in seeds]) == [[v] for v in seeds]


def test_order_of_every_component_of_48_maps():
    """A few blobs per 8^3 map, every component of every map in one call, asked for in shuffled order from a seed drawn here."""
    rng = np.random.default_rng(48)
    maps = [ref.blobs(8, 2 + k % 4, rng) for k in range(48)]
    asked = []
    for k, m in enumerate(maps):
        for members in ref.components(m).values():
            asked.append((k, int(rng.choice(members)), len(members)))
    assert len(asked) > 96 and max(a[2] for a in asked) > 30
    asked = [asked[i] for i in rng.permutation(len(asked))]
    with density(maps) as handle:
        got = device_order(handle, asked)
    for (k, seed, _), members in zip(asked, got):
        assert members == ref.bfs_order(maps[k], seed), (k, seed)


# -------------------------------------------------------------------------------------------------------------------------- calls
@functools.lru_cache(maxsize=None)
def call_case():
    """A 16^3 map of blobs and specks, its components [(0, seed, size)] largest first and their member lists."""
    rng = np.random.default_rng(16)
    m = ref.blobs(16, 7, rng, speck=0.004)
    m.flags.writeable = False
    comps = sorted(ref.components(m).values(), key=len, reverse=True)
    asked = [(0, int(c[len(c) // 2]), len(c)) for c in comps]
    assert len(asked) >= 6 and asked[0][2] >= 40 and asked[1][2] >= 8
    return m, asked, [ref.bfs_order(m, seed) for _, seed, _ in asked]


def test_a_second_call_gives_the_same_lists_and_a_partial_call_its_own():
    m, asked, want = call_case()
    with density([m]) as handle:
        first = device_order(handle, asked)
        assert first == want
        assert device_order(handle, asked) == first  # the claims of the first call are gone
        assert device_order(handle, asked[::2]) == want[::2]
        assert device_order(handle, asked[1::2][::-1]) == want[1::2][::-1]
        assert device_order(handle, []) == []  # PMX_OK, and the buffer untouched (device_order checks it)
        assert device_order(handle, asked) == first


def test_slices_longer_and_shorter_than_the_component():
    m, asked, want = call_case()
    with density([m]) as handle:
        longer = [(k, seed, n + 5) for k, seed, n in asked[:3]]
        assert device_order(handle, longer) == [w + [-1] * 5 for w in want[:3]]
        # the first slice too short by half: whatever it holds is the member that belongs at that place or -1, and the next list is whole
        short = [(0, asked[0][1], asked[0][2] // 2), asked[1]]
        got = device_order(handle, short)
        assert got[1] == want[1]
        assert len(got[0]) == asked[0][2] // 2 and got[0][0] == asked[0][1]
        assert all(g == -1 or g == w for g, w in zip(got[0], want[0]))
        assert device_order(handle, asked) == want  # and the handle serves the next call


def test_refusals_of_create():
    lib = libpmx()
    one = np.full(8, 0.5, dtype=np.float32)
    for n_maps, size in ((1, 0), (1, 129), (0, 2), (1024, 128)):  # (the last: 2^31 voxels, refused before anything is allocated or read)
        handle = ctypes.c_void_p()
        assert lib.pmx_density_create(one.ctypes.data, n_maps, size, 0, ctypes.byref(handle)) == 1
        assert b"pmx_density_create" in lib.pmx_last_error()
        assert not handle.value
    with density([one.reshape(2, 2, 2)]) as handle:  # the next valid call is served
        assert device_labels(handle, 1, 2)[0].tolist() == [0] * 8


def test_refusals_of_order():
    m, asked, want = call_case()
    size = asked[0][2]
    two = asked[:2]
    sizes = [0, asked[0][2], asked[0][2] + asked[1][2]]
    with density([m, m]) as handle:
        for comps, offsets in (
            (two, [1, sizes[1] + 1, sizes[2] + 1]),  # comp_offset[0] != 0
            (two, [0, 0, sizes[2]]),  # an empty slice
            (two, [0, sizes[1], sizes[1]]),
            ([(-1, asked[0][1], size)], None),  # comp_map out of range
            ([(2, asked[0][1], size)], None),
            ([asked[0], (0, -1, 4)], None),  # a seed outside the map
            ([asked[0], (1, 16**3, 4)], None),
        ):
            assert device_order(handle, comps, offsets=offsets, status=1) is None
            assert device_order(handle, [asked[0], (1, asked[1][1], asked[1][2])]) == want[:2]  # the next valid call is served


# -------------------------------------------------------------------------------------------------------------------- the wrapper
def assert_wrapper_equals_host_search(masks):
    from pharmaconet_amd.model_builder import voxel_components, voxel_components_device

    got = voxel_components_device(masks, 0)
    assert len(got) == len(masks)
    n_comp = 0
    for m, comps in zip(masks, got):
        want = list(voxel_components(m))
        assert len(comps) == len(want)
        for (gm, gv), (wm, wv) in zip(comps, want):
            assert gm.tolist() == [list(p) for p in wm]
            assert gv.tolist() == wv
        n_comp += len(want)
    return n_comp


@pytest.mark.parametrize("name", ("mixed24", "charged40", "crowded48"))
def test_wrapper_equals_the_host_search_on_the_fixture_maps(name):
    from test_model_builder import load_inputs

    masks = [info["point_map"] for info in load_inputs(name)[1]]
    assert assert_wrapper_equals_host_search(masks) > len(masks)


def test_wrapper_equals_the_host_search_at_size_24():
    rng = np.random.default_rng(24)
    masks = [ref.blobs(24, 10 + 3 * k, rng, speck=0.002) for k in range(5)] + [np.zeros((24, 24, 24), dtype=np.float32)]
    assert assert_wrapper_equals_host_search(masks) > 40


def test_wrapper_refuses_a_map_that_changes_in_float32():
    from pharmaconet_amd.model_builder import voxel_components_device

    m = np.zeros((8, 8, 8), dtype=np.float64)
    m[2, 2, 2:5] = (0.5, 1e-50, 0.5)  # active in float64, zero in float32
    with pytest.raises(RuntimeError, match="cast to float32"):
        voxel_components_device([m], 0)
    m[2, 2, 3] = 1e-40  # a float32 subnormal: the same voxels either way
    got = voxel_components_device([m], 0)[0]
    assert len(got) == 1 and sorted(got[0][0].tolist()) == [[2, 2, 2], [2, 2, 3], [2, 2, 4]]
