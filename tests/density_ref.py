"""Plain restatement of what `csrc/pmx_density.hip` computes, and the voxel shapes its tests walk.

`labels_ref`: the smallest linear index of each voxel's 26-connected component of `mask > 0` (what `dm_label_kernel` writes);
`bfs_order`: a component's voxels in the reference's breadth-first discovery order from a GIVEN seed (`utils/density_map.py:93-109`,
what `dm_order_kernel` writes) - the host search of `model_builder.voxel_components` with the seed taken out of CPython's hands;
`bfs_levels`: the width of every level of that search, i.e. the frontier widths the order kernel's scan sees.
Pure Python / NumPy on coordinates: no linear-index neighbour arithmetic, so nothing here can wrap into the next row, plane or map.
tests/test_density_cpu.py pins all three to `voxel_components` and to literal cases."""

from __future__ import annotations

import itertools

import numpy as np

STEPS = tuple(s for s in itertools.product((-1, 0, 1), repeat=3) if s != (0, 0, 0))


def _active(mask):
    m = np.asarray(mask)
    assert m.ndim == 3 and m.shape[0] == m.shape[1] == m.shape[2]
    return m.astype(np.float32, copy=False) > np.float32(0.0)  # NumPy's comparison on float32: subnormals and +inf are active


def linear(p, size):
    return (p[0] * size + p[1]) * size + p[2]


def coords(v, size):
    return (v // (size * size), (v // size) % size, v % size)


def _search(on, size, seed):
    """Members (coordinate tuples) in discovery order and the index in that list at which every level starts."""
    members, seen = [seed], {seed}
    starts, head, level_end = [0], 0, 1
    while head < len(members):
        if head == level_end:
            starts.append(head)
            level_end = len(members)
        x, y, z = members[head]
        head += 1
        for dx, dy, dz in STEPS:
            qx, qy, qz = x + dx, y + dy, z + dz
            if 0 <= qx < size and 0 <= qy < size and 0 <= qz < size and on[qx, qy, qz]:
                q = (qx, qy, qz)
                if q not in seen:
                    seen.add(q)
                    members.append(q)
    return members, starts


def _seed(seed, size):
    seed = coords(int(seed), size) if np.ndim(seed) == 0 else tuple(int(c) for c in seed)
    assert all(0 <= c < size for c in seed)
    return seed


def bfs_order(mask, seed) -> list[int]:
    """Linear indices of the seed's component in discovery order: the queue is the member list, a voxel's neighbours are tried in
    itertools.product((-1, 0, 1), repeat=3) order without the centre. `seed`: (x, y, z) or a linear index; it must be active."""
    on = _active(mask)
    size = on.shape[0]
    seed = _seed(seed, size)
    assert on[seed], "the seed is not an active voxel"
    return [linear(p, size) for p in _search(on, size, seed)[0]]


def bfs_levels(mask, seed) -> list[int]:
    """Width of every breadth-first level from `seed` (level 0 is the seed alone)."""
    on = _active(mask)
    size = on.shape[0]
    members, starts = _search(on, size, _seed(seed, size))
    return np.diff(starts + [len(members)]).tolist()


def labels_ref(mask) -> np.ndarray:
    """int32 [S^3]: the smallest linear index (x * S + y) * S + z of each voxel's 26-connected component of `mask > 0`, -1 elsewhere."""
    on = _active(mask)
    size = on.shape[0]
    out = np.full(size**3, -1, dtype=np.int32)
    for v in np.flatnonzero(on.reshape(-1)).tolist():  # ascending: the first voxel of a component met is its smallest index
        if out[v] < 0:
            out[[linear(p, size) for p in _search(on, size, coords(v, size))[0]]] = v
    return out


def components(mask) -> dict[int, np.ndarray]:
    """label -> the ascending linear indices of that component."""
    lab = labels_ref(mask)
    return {int(l): np.flatnonzero(lab == l) for l in np.unique(lab[lab >= 0])}


# ------------------------------------------------------------------------------------------------------------------------- shapes
def _values(on):
    """float32 map: a positive value that differs from voxel to voxel where `on`, 0 elsewhere."""
    v = np.arange(on.size, dtype=np.int64).reshape(on.shape)
    return np.where(on, 0.05 + ((v * 7919) % 1009) / 1009.0, 0.0).astype(np.float32)


def prism(size, n):
    """The first n cells of the (y, z) plane sorted by (max(y, z), y, z), extruded along the whole x axis: searched from (0, 0, 0),
    every level past the cross-section's half-width is one whole x-slice - exactly n voxels."""
    cells = sorted(itertools.product(range(size), repeat=2), key=lambda c: (max(c), c[0], c[1]))[:n]
    assert len(cells) == n
    on = np.zeros((size, size, size), dtype=bool)
    for y, z in cells:
        on[:, y, z] = True
    return _values(on)


def snake_path(size):
    """The voxels of `snake(size)` in path order, from (0, 0, 0)."""
    assert size % 2 == 0 and size >= 4
    path = []
    z_up, y_up = True, True
    for x in range(0, size, 2):
        ys = list(range(0, size, 2)) if y_up else list(range(size - 2, -1, -2))
        for k, y in enumerate(ys):
            zs = list(range(size)) if z_up else list(range(size - 1, -1, -1))
            path += [(x, y, z) for z in zs]
            z_up = not z_up
            if k + 1 < len(ys):
                path.append((x, (y + ys[k + 1]) // 2, zs[-1]))  # the one voxel that joins this row to the next
        if x + 2 < size:
            path.append((x + 1, ys[-1], path[-1][2]))  # the one voxel that joins this plane to the next
        y_up = not y_up
    return path


def snake(size):
    """One 26-connected component that is a single path: full z-rows on every second y of every second x-plane, consecutive rows and
    planes joined by single voxels at alternating ends; no two rows touch."""
    on = np.zeros((size, size, size), dtype=bool)
    for p in snake_path(size):
        on[p] = True
    return _values(on)


def snake_variants(size):
    """name -> the snake, flipped and axis-permuted: the component's smallest linear index (where every label ends up) sits at an end
    of the path (`plain`), at its other end region (`flip_x`), inside it (`flip_y`, `flip_all`) and, with the rows along x or y, on
    a row that the sweep order of the label kernel crosses instead of follows (`zyx`, `yzx`, `xzy_flip`)."""
    s = snake(size)
    out = {
        "plain": s,
        "flip_x": s[::-1],
        "flip_y": s[:, ::-1],
        "flip_all": s[::-1, ::-1, ::-1],
        "zyx": s.transpose(2, 1, 0),
        "yzx": s.transpose(1, 2, 0),
        "xzy_flip": s.transpose(0, 2, 1)[::-1, :, ::-1],
    }
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


def lattice(size):
    """Every voxel with all-even coordinates: ceil(S / 2)^3 components of one voxel."""
    on = np.zeros((size, size, size), dtype=bool)
    on[::2, ::2, ::2] = True
    return _values(on)


def full(size):
    return _values(np.ones((size, size, size), dtype=bool))


def wrap_traps(size):
    """Pairs adjacent in linear index that are no neighbours: (0, 0, S-1) with (0, 1, 0) - the end of a row and the start of the
    next - and (1, S-1, 2) with (2, 0, 2) - one row stride apart across two planes. Four components of one voxel."""
    assert size >= 4
    on = np.zeros((size, size, size), dtype=bool)
    on[0, 0, size - 1] = on[0, 1, 0] = on[1, size - 1, 2] = on[2, 0, 2] = True
    return _values(on)


def wrap_trap_stack(size, n_maps):
    """[n_maps, S, S, S]: the last voxel of every map and the first voxel of every map - in a stack, the last voxel of map m and the
    first of map m + 1 are adjacent in memory."""
    assert size >= 3
    on = np.zeros((n_maps, size, size, size), dtype=bool)
    on[:, 0, 0, 0] = on[:, -1, -1, -1] = True
    return np.stack([_values(m) * np.float32(1 + k) for k, m in enumerate(on)])


def blobs(size, n, rng, speck=0.0):
    """n random balls (they may touch through faces, edges and corners, and the grid's faces cut them) with random positive values,
    plus single voxels with probability `speck`."""
    g = np.stack(np.meshgrid(*[np.arange(size)] * 3, indexing="ij"), -1)
    m = np.zeros((size, size, size), dtype=np.float32)
    for _ in range(n):
        c = rng.integers(0, size, size=3)
        r = rng.uniform(0.8, max(1.0, min(5.5, size / 4)))
        inside = ((g - c) ** 2).sum(-1) <= r * r
        m[inside] = rng.uniform(0.05, 1.0, size=int(inside.sum())).astype(np.float32)
    if speck:
        m[rng.random(m.shape) < speck] = 0.3
    return m
