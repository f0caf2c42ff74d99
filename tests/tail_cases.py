"""Builders shared by the tail tests: tests/test_gpu_tails.py (self entries), tests/test_gpu_pair_tails.py (pair entries),
tests/test_gpu_tail_shapes.py and tests/test_gpu_explain_shapes.py (both arms at every lane shape) run them on the GPU,
tests/test_tail_cases_cpu.py checks from the oracle alone that the libraries reach what those tests are about. The cases of the lane-shape
tests are computed once per process, shared, and never written to."""

import dataclasses
import functools
import itertools
import os
import struct

import numpy as np

from conftest import GOLDEN

FLOOR = 1e-30
THREADS = min(os.cpu_count() or 8, 16)
# conformers per ligand: G = 1 ... 64 (G = 2^ceil(log2 C)), groups full and partly filled
SHAPES = (1, 2, 3, 4, 12, 16, 20, 32, 33, 48, 64)

WEIGHT_SETS = {
    "default": None,
    "charged_heavy": {"Cation": 100.0, "Anion": 100.0, "Hydrophobic": 0.1},  # VERDICT r4's example (--cation 100 --hydrophobic 0.1)
    "charged_light": {"Cation": 0.1, "Anion": 0.1, "Hydrophobic": 100.0},   # ... and its inverse
    # types that share clusters in the fixture models (Cation + HBond, Aromatic + Hydrophobic) a factor 1000 apart
    "core_heavy": {"Cation": 100.0, "Anion": 100.0, "Aromatic": 100.0, "HBond_donor": 0.1, "HBond_acceptor": 0.1, "Hydrophobic": 0.1, "Halogen": 0.1},
    "core_light": {"Cation": 0.1, "Anion": 0.1, "Aromatic": 0.1, "HBond_donor": 100.0, "HBond_acceptor": 100.0, "Hydrophobic": 100.0, "Halogen": 100.0},
}


class _Shim:
    """What engine.screen needs of a model: `.flat` and a slot for the device handle."""

    def __init__(self, flat):
        self.flat = flat
        self._engine_handle = None


# ------------------------------------------------------------------------------------------------ pair entries (test_gpu_pair_tails.py)
def _record(masks_a, masks_b, xyz: np.ndarray) -> bytes:
    """Two ligand clusters (nodes of `masks_a`, then of `masks_b`); xyz float32 [n][3][C]."""
    n, C = xyz.shape[0], xyz.shape[2]
    head = struct.pack("<HHHH", n, C, 2, 0) + bytes(list(masks_a) + list(masks_b)) + bytes([len(masks_a), n])
    head += b"\0" * (-len(head) % 4)
    rec = head + np.ascontiguousarray(xyz, dtype=np.float32).tobytes()
    return rec + b"\0" * (-len(rec) % 16)


def _subsets(flat, a: int):
    """Distinct non-empty node subsets of model cluster `a` by ligand type mask (graph_match.py:148-150): {node tuple: mask}."""
    nodes = int(np.asarray(flat.cluster_nodes).reshape(flat.num_clusters, -1)[a, 0])
    subs = {}
    for mask in range(1, 128):
        sub = tuple(m for m in range(flat.num_nodes) if (nodes >> m) & 1 and (mask >> int(flat.node_type[m])) & 1)
        if sub and sub not in subs:
            subs[sub] = mask
    return subs


def _two_cluster_model(flat, a: int, b: int):
    """The model reduced to clusters a and b (all nodes and edges kept, so node indices stand)."""
    idx = [a, b]
    return dataclasses.replace(
        flat,
        cluster_nodes=np.asarray(flat.cluster_nodes)[idx].copy(),
        cluster_typemask=flat.cluster_typemask[idx].copy(),
        cluster_center=flat.cluster_center[idx].copy(),
        cluster_size=flat.cluster_size[idx].copy(),
        cluster_type=tuple(flat.cluster_type[i] for i in idx),
    )


def _pin(flat, A, B):
    """A distance at which the item of node subsets (A, B) passes the majority test of match_utils.py:55-61 (the edge mean that
    most terms lie within 2 sigma of), or None."""
    mean = flat.edge_mean.astype(np.float32)
    std = flat.edge_std.astype(np.float32)
    best, best_d = -1, None
    for m, n in itertools.product(A, B):
        d = np.float32(mean[m, n])
        if not np.isfinite(d):
            continue
        cnt = sum(1 for mm, nn in itertools.product(A, B) if abs(np.float32(d - mean[mm, nn]) / std[mm, nn]) < 2.0)
        if cnt > best:
            best, best_d = cnt, float(d)
    if best_d is None or 2 * best < len(A) * len(B):
        return None
    return best_d


def _heavy_light(flat, a, w7):
    """The node subsets of cluster `a` made of its heaviest-weighted type only and of its lightest only: ((nodes, mask), (nodes, mask)) or None."""
    subs = _subsets(flat, a)
    ws = sorted({w7[int(flat.node_type[m])] for sub in subs for m in sub})
    if len(ws) < 2:
        return None
    pick = {}
    for sub, mask in subs.items():
        kinds = {w7[int(flat.node_type[m])] for m in sub}
        for name, w in (("H", ws[-1]), ("L", ws[0])):
            if kinds == {w} and (name not in pick or len(sub) > len(pick[name][0])):
                pick[name] = (sub, mask)
    return (pick["H"], pick["L"]) if len(pick) == 2 else None


def _rescaled(flat, sigma_min_to: float):
    """The same model with every length multiplied so that its smallest edge sigma is `sigma_min_to` - just above a power of two, the
    tabulated functions' grid (h = the largest power of two <= sigma_min / 4) is as coarse against the sigmas as it can get."""
    f = np.float64(sigma_min_to) / np.float64(np.nanmin(flat.edge_std))
    return dataclasses.replace(
        flat,
        edge_mean=(flat.edge_mean.astype(np.float64) * f).astype(np.float32),
        edge_std=(flat.edge_std.astype(np.float64) * f).astype(np.float32),
        cluster_center=flat.cluster_center * f,
        cluster_size=flat.cluster_size * f,
    )


def heavy_tail_library(flat, w7, a, b, n_conf, n_dist=1600, rng=None):
    """Ligands of two clusters of three light-typed nodes and one heavy-typed node each, against model clusters (a, b): the nine light x light
    node pairs sit where their function passes, the six heavy x light ones 12 of the largest sigma away (they fail and add nothing), and
    the one heavy x heavy pair is swept over `n_dist` distances from 2 sigma inside its mean to 10 sigma beyond, `n_conf` of them per
    record: record j holds distances (j * n_conf + arange(n_conf)) * step. None where the cluster pair has no heavy and light subsets
    under `w7`, or no distance at which their items pass. `rng` draws the light nodes' jitter (one draw per library, after those checks)."""
    from pharmaconet_amd import PackedLibrary

    ha, hb = _heavy_light(flat, a, w7), _heavy_light(flat, b, w7)
    if ha is None or hb is None:
        return None
    (Ha, mHa), (La, mLa) = ha
    (Hb, mHb), (Lb, mLb) = hb
    p_ll, p_hh = _pin(flat, La, Lb), _pin(flat, Ha, Hb)
    if p_ll is None or p_hh is None:
        return None
    if rng is None:
        rng = np.random.default_rng(7)
    far = 12.0 * float(np.nanmax(flat.edge_std))  # where the heavy nodes sit, off the axis of the light ones
    step = 0.0125 * float(np.nanmin(flat.edge_std)) / 1.4
    jit = rng.normal(size=(2, 3, 3)) * 0.14 * float(np.nanmin(flat.edge_std))
    recs = []
    for j in range(-(-n_dist // n_conf)):
        t = np.maximum(p_hh - 240 * step + (j * n_conf + np.arange(n_conf)) * step, 0.05)  # the heavy pair, from 2 sigma inside its mean to 10 sigma beyond
        xyz = np.zeros((8, 3, n_conf))
        for k in range(3):
            xyz[k] = jit[0, k][:, None]
            xyz[4 + k] = jit[1, k][:, None]
            xyz[4 + k, 0, :] += p_ll
        xyz[3, 0, :], xyz[3, 1, :] = p_ll / 2 - t / 2, far
        xyz[7, 0, :], xyz[7, 1, :] = p_ll / 2 + t / 2, far
        recs.append(_record([mLa] * 3 + [mHa], [mLb] * 3 + [mHb], xyz.astype(np.float32)))
    return PackedLibrary.from_records(recs)


# ------------------------------------------------------------------------------------------------ self entries (test_gpu_tails.py)
def _two_node_record(mask1: int, mask2: int, d: np.ndarray) -> bytes:
    """One cluster of two nodes, node 0 at the origin and node 1 at (d[c], 0, 0) in conformer c."""
    C = len(d)
    xyz = np.zeros((2, 3, C), dtype=np.float32)
    xyz[1, 0, :] = d
    head = struct.pack("<HHHH", 2, C, 1, 0) + bytes([mask1, mask2]) + bytes([2])
    head += b"\0" * (-len(head) % 4)
    rec = head + xyz.tobytes()
    return rec + b"\0" * (-len(rec) % 16)


def _subset_pairs(flat, a: int):
    """Distinct non-empty node subsets of model cluster `a` by ligand type mask (graph_match.py:148-150), one mask each, and
    every unordered pair of them (the same subset twice included: two ligand nodes of one type)."""
    nodes = int(flat.cluster_nodes[a])
    subs = {}
    for mask in range(1, 128):
        sub = 0
        for m in range(flat.num_nodes):
            if (nodes >> m) & 1 and (mask >> int(flat.node_type[m])) & 1:
                sub |= 1 << m
        if sub and sub not in subs:
            subs[sub] = mask
    masks = list(subs.values())
    return [(masks[i], masks[j]) for i in range(len(masks)) for j in range(i, len(masks))]


def _single_cluster_model(flat, a: int):
    """The model reduced to cluster `a` (all nodes and edges kept, so node indices stand): the two-node ligand then has one
    level with one candidate, and its score is the mean over conformers of max(0, S[0][a])."""
    return dataclasses.replace(
        flat,
        cluster_nodes=flat.cluster_nodes[a:a + 1].copy(),
        cluster_typemask=flat.cluster_typemask[a:a + 1].copy(),
        cluster_center=flat.cluster_center[a:a + 1].copy(),
        cluster_size=flat.cluster_size[a:a + 1].copy(),
        cluster_type=tuple(flat.cluster_type[a:a + 1]),
    )


def _sweep_library(pairs, dmax: float, n_conf: int, delta: float):
    """For every mask pair, ligands whose conformers step through [0, dmax] in `delta` increments."""
    from pharmaconet_amd import PackedLibrary

    per = int(np.ceil(dmax / (delta * n_conf)))
    recs, dist = [], []
    for m1, m2 in pairs:
        for j in range(per):
            d = ((j * n_conf + np.arange(n_conf)) * delta).astype(np.float32)
            recs.append(_two_node_record(m1, m2, d))
            dist.append(d)
    return PackedLibrary.from_records(recs), np.array(dist)


def _table_range(flat) -> float:
    return float(np.nanmax(flat.edge_mean.astype(np.float64) + 7.0 * flat.edge_std.astype(np.float64)))


# ------------------------------------------------------------------------------------------------ the cases of the lane-shape tests
# The coarsest grids of test_one_heavy_item_in_the_tails_beside_light_items_that_pass: there the tabulated tail alone is off by 1e-5.
PAIR_SHAPE_SETS = (("core_heavy", 1.0000005), ("core_light", 2.000001))
PAIR_SHAPE_PAIRS = 6
SELF_SHAPES = tuple(C for C in SHAPES if C != 1)  # (C = 8 and C = 1 are test_gpu_tails.py's full sweeps)
SELF_SHAPE_CLUSTERS = 3
SELF_SHAPE_DELTA = 0.05


def _fixture_flat():
    from pharmaconet_amd import PharmacophoreModel

    return PharmacophoreModel.load(GOLDEN / "model_6oim_like.pm").flat


@dataclasses.dataclass
class PairShapeCase:
    """One cluster pair of a lane shape: the two-cluster model, its `heavy_tail_library`, and the oracle's scores and statistics."""

    a: int
    b: int
    flat: object
    lib: object
    ref: np.ndarray
    stats: np.ndarray

    @property
    def valid(self):
        """Records with a valid pair entry."""
        return self.stats["p_entries"] - self.stats["p_invalid"] > 0

    @property
    def mostly_tail(self):
        """Records that are mostly the one heavy tail item: above the far end of the sweep (the light items alone), below 50 times it."""
        floor_score = self.ref.min()
        return (self.ref > 1.05 * floor_score) & (self.ref < 50 * floor_score)


@functools.lru_cache(maxsize=None)
def pair_shape_cases(wname: str, sigma_min_to: float, n_conf: int):
    """The rescaled fixture model's first PAIR_SHAPE_PAIRS cluster pairs (a, b), in the double-loop order of
    test_one_heavy_item_in_the_tails_beside_light_items_that_pass, that have a `heavy_tail_library` under the weight set."""
    from oracle import oracle
    from pharmaconet_amd.constants import weights_vector

    flat = _rescaled(_fixture_flat(), sigma_min_to)
    w7 = weights_vector(WEIGHT_SETS[wname])
    out = []
    for a, b in itertools.permutations(range(flat.num_clusters), 2):
        lib = heavy_tail_library(flat, w7, a, b, n_conf)
        if lib is None:
            continue
        sub = _two_cluster_model(flat, a, b)
        ref, stats = oracle.oracle_score(sub, lib, w7, num_threads=THREADS, with_stats=True)
        out.append(PairShapeCase(a, b, sub, lib, ref, stats))
        if len(out) == PAIR_SHAPE_PAIRS:
            break
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pair_shape_explained(wname: str, sigma_min_to: float, n_conf: int):
    """`oracle_explain` at two modes of every library of `pair_shape_cases`, in its order."""
    from oracle import oracle
    from pharmaconet_amd.constants import weights_vector

    w7 = weights_vector(WEIGHT_SETS[wname])
    return tuple(oracle.oracle_explain(c.flat, c.lib, w7, n_modes=2, num_threads=THREADS) for c in pair_shape_cases(wname, sigma_min_to, n_conf))


@dataclasses.dataclass
class SelfShapeCase:
    """One cluster of a lane shape: the single-cluster model, its `_sweep_library`, and the oracle's scores."""

    a: int
    flat: object
    lib: object
    ref: np.ndarray


@functools.lru_cache(maxsize=None)
def self_shape_cases(n_conf: int):
    """The fixture model's SELF_SHAPE_CLUSTERS clusters with the most subset pairs (the first of equals), each swept to 5 A beyond the table range."""
    from oracle import oracle
    from pharmaconet_amd.constants import weights_vector

    flat = _fixture_flat()
    pairs = {a: _subset_pairs(flat, a) for a in range(flat.num_clusters)}
    out = []
    for a in sorted(pairs, key=lambda a: -len(pairs[a]))[:SELF_SHAPE_CLUSTERS]:
        sub = _single_cluster_model(flat, a)
        lib, _ = _sweep_library(pairs[a], _table_range(flat) + 5.0, n_conf, SELF_SHAPE_DELTA)
        out.append(SelfShapeCase(a, sub, lib, oracle.oracle_score(sub, lib, weights_vector(None), num_threads=THREADS)))
    return tuple(out)
