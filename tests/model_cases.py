"""Hand-made models and the ligands that aim at them, shared by tests/test_model_cases_cpu.py (which checks from the oracle and the host
tables alone that every case reaches what it is about) and tests/test_gpu_hand_models.py (which runs them on the GPU):

  A  models whose edge matrix is not symmetric: the square function index of the table phase, the SWAP arm of csrc/pmx_rows.hip
  B  cells of a tabulated function whose pass set is two windows: the term-by-term majority count, `n_exact_cells`
  C  the floats next to the ends of an edge's 2-sigma window, on the golden models
  D  a model of 256 nodes and 128 clusters, the header's limits

Every ligand is written by the record writers of tests/tail_cases.py with its nodes on the x axis, the swept node at (d, 0, 0): the
float32 distance both the engine and the oracle compute is sqrt(d * d) = d itself. An asymmetric edge is read as oracle/pmx_oracle.c
`node_pair_term(a, b)` reads it, `edge[a.m * Nm + b.m]`, with a before b in a cluster's iteration order (self entries) or a from the earlier
tree level (pair entries). Every case's oracle scores are computed once per process and are read-only."""

import ctypes
import dataclasses
import functools
import itertools

import numpy as np

from conftest import GOLDEN, load_golden
from tail_cases import THREADS, _pin, _record, _single_cluster_model, _subsets, _two_cluster_model, _two_node_record
from test_model_tables_cpu import HAND_MODELS, TablesView, build_tables, cluster_lists, down, function_pairs, hand_model, subset_nodes, up

F32 = np.float32
CONFORMERS = (1, 3, 8, 33, 64)  # A1, A2: G = 1, 4, 8, 64 with groups full and partly filled
SWEEP_STEP = 0.05
# A3: the upper triangle's means times 1 + 0.05 u, its stds times 1 + 0.2 v (u, v uniform in [-1, 1]); the factors the issue gives reach the
# share of rows test_model_cases_cpu.py asks for (the measured shares are in its docstring), so they stand
A3_MEAN_FACTOR, A3_STD_FACTOR = 0.05, 0.2


@dataclasses.dataclass(frozen=True, eq=False)
class Case:
    """One model with one library: `ref` the oracle's scores [records], `dist` the swept distances [records, C] (None where the ligands are
    golden ones), `aim` what the case is aimed at (per family, see the builders)."""

    name: str
    flat: object
    lib: object
    ref: np.ndarray
    dist: object = None
    aim: object = None


def _frozen(a):
    a = np.asarray(a)
    a.flags.writeable = False
    return a


def oracle_scores(flat, lib):
    from oracle import oracle
    from pharmaconet_amd.constants import weights_vector

    return _frozen(oracle.oracle_score(flat, lib, weights_vector(None), num_threads=THREADS))


def transposed(flat):
    """The model with edge (m, n) and edge (n, m) exchanged."""
    return dataclasses.replace(flat, edge_mean=np.ascontiguousarray(flat.edge_mean.T), edge_std=np.ascontiguousarray(flat.edge_std.T))


# ------------------------------------------------------------------------------------------------ host tables
@functools.lru_cache(maxsize=None)
def host_lib():
    """The host-only library's private `pmxt_*` hook, as the `hook` fixture of tests/test_model_tables_cpu.py opens it."""
    import __graft_entry__ as entry

    entry.build()
    from pharmaconet_amd import _ffi

    lib = ctypes.CDLL(str(_ffi.LIB_PATH.with_name("libpmx_pack.so")))
    lib.pmxt_tables_create.argtypes = [ctypes.POINTER(_ffi.ModelDesc), ctypes.POINTER(ctypes.c_void_p)]
    lib.pmxt_tables_view_get.argtypes = [ctypes.c_void_p, ctypes.POINTER(TablesView)]
    lib.pmxt_tables_destroy.argtypes = [ctypes.c_void_p]
    lib.pmx_last_error.restype = ctypes.c_char_p
    return lib


def host_tables(flat):
    return build_tables(host_lib(), flat)


@functools.lru_cache(maxsize=None)
def golden_flat(name):
    from pharmaconet_amd import PharmacophoreModel

    return PharmacophoreModel.load(GOLDEN / f"{name}.pm").flat


def fn_id(t, sa, sb):
    """The function of subsets (sa, sb) in tables `t`."""
    if t["symmetric"]:
        hi, lo = max(sa, sb), min(sa, sb)
        return hi * (hi + 1) // 2 + lo
    return sa * t["NS"] + sb


def cell_of(t, d):
    return np.minimum((np.asarray(d, F32) / F32(t["h"])).astype(np.int64), t["ncell"] - 1)


def aimed_windows(flat, m0, m1):
    """For the two-cluster model `flat` and ligand clusters of one node each, masks m0 (level 0, model cluster 0) and m1 (level 1, model
    cluster 1): (tables, the function's rows of `win` [ncell, 2])."""
    t = host_tables(flat)
    sa, sb = int(t["sidtab"][0 * 128 + m0]), int(t["sidtab"][1 * 128 + m1])
    assert sa and sb
    return t, t["win"][fn_id(t, sa, sb)]


# ------------------------------------------------------------------------------------------------ record packing
def pair_record(m0, m1, d):
    """Two ligand clusters of one node each: mask m0 at the origin, mask m1 at (d[c], 0, 0) in conformer c."""
    xyz = np.zeros((2, 3, len(d)), dtype=np.float32)
    xyz[1, 0, :] = d
    return _record([m0], [m1], xyz)


def steps(dmax, n_conf):
    """0, 0.05, ... to dmax and on to the end of the last record, as tail_cases._sweep_library packs them: [records, n_conf] float32."""
    per = -(-(int(np.ceil(dmax / SWEEP_STEP)) + 1) // n_conf)
    return ((np.arange(per * n_conf) * SWEEP_STEP).astype(np.float32)).reshape(per, n_conf)


def in_records(d, n_conf):
    """The sweep `d` in its order, n_conf floats per record (the last record filled up with the last float): [records, n_conf]."""
    d = np.asarray(d, dtype=np.float32)
    pad = -len(d) % n_conf
    return np.concatenate([d, np.full(pad, d[-1], dtype=np.float32)]).reshape(-1, n_conf)


def library(writer, mask_pairs, dist):
    """`writer(m0, m1, d)` for every mask pair and every row of `dist`: (PackedLibrary, dist tiled [records, C], mask pair of every record)."""
    from pharmaconet_amd import PackedLibrary

    recs = [writer(m0, m1, row) for m0, m1 in mask_pairs for row in dist]
    which = np.repeat(np.arange(len(mask_pairs)), len(dist))
    return PackedLibrary.from_records(recs), _frozen(np.tile(dist, (len(mask_pairs), 1))), _frozen(which)


def around(x, n):
    """The 2 n + 1 floats from n ulps below x to n ulps above (none below 0)."""
    x = F32(x)
    below, above = [], []
    lo = hi = x
    for _ in range(n):
        lo, hi = down(lo), up(hi)
        below.append(lo)
        above.append(hi)
    out = np.array(below[::-1] + [x] + above, dtype=np.float32)
    return out[out >= 0]


def table_range(flat):
    return float(np.nanmax(flat.edge_mean.astype(np.float64) + 7.0 * flat.edge_std.astype(np.float64)))


# ------------------------------------------------------------------------------------------------ A: asymmetric models
def asym3():
    return HAND_MODELS["asym3"]()


def a1_mask_pairs(flat):
    """Every ordered pair of type masks (one per distinct set of the model's types) that selects non-empty subsets in two different clusters."""
    types = sorted({int(x) for x in flat.node_type})
    masks = [sum(1 << types[i] for i in range(len(types)) if bits >> i & 1) for bits in range(1, 1 << len(types))]
    reach = {m: {a for a, nodes in enumerate(cluster_lists(flat)) if any(m >> int(flat.node_type[n]) & 1 for n in nodes)} for m in masks}
    return [(m0, m1) for m0 in masks for m1 in masks if any(a != b for a in reach[m0] for b in reach[m1])]


@functools.lru_cache(maxsize=None)
def a1_cases():
    """`asym3` against two-cluster ligands of one node each, one Case per conformer count; aim = (mask pairs, mask pair of every record)."""
    flat = asym3()
    pairs = a1_mask_pairs(flat)
    out = []
    for C in CONFORMERS:
        lib, dist, which = library(pair_record, pairs, steps(table_range(flat), C))
        out.append(Case(f"a1_c{C}", flat, lib, oracle_scores(flat, lib), dist, (tuple(pairs), which)))
    return tuple(out)


A2_MASKS = {0: ((1, 1),), 2: ((1, 16), (16, 1))}  # cluster {0, 1}: one type, both subsets {0, 1}; cluster {0, 2}: subsets {0} and {2}, both node orders


@functools.lru_cache(maxsize=None)
def a2_cases():
    """`asym3` reduced to one cluster, against two-node ligands; aim = (cluster, whether the two nodes have one type)."""
    full = asym3()
    out = []
    for a, pairs in A2_MASKS.items():
        flat = _single_cluster_model(full, a)
        for C in CONFORMERS:
            lib, dist, _ = library(_two_node_record, pairs, steps(table_range(full), C))
            out.append(Case(f"a2_cluster{a}_c{C}", flat, lib, oracle_scores(flat, lib), dist, (a, pairs[0][0] == pairs[0][1])))
    return tuple(out)


def asym_scaled(flat, mean_factor=A3_MEAN_FACTOR, std_factor=A3_STD_FACTOR):
    """`flat` with the upper triangle (m < n) of its means times 1 + mean_factor u and of its stds times 1 + std_factor v, u and v uniform
    in [-1, 1] from default_rng(1); rounded to float32; diagonal and lower triangle as they are."""
    rng = np.random.default_rng(1)
    nm = flat.num_nodes
    u, v = rng.uniform(-1.0, 1.0, (nm, nm)), rng.uniform(-1.0, 1.0, (nm, nm))
    upper = np.triu(np.ones((nm, nm), dtype=bool), 1)
    mean = np.where(upper, flat.edge_mean.astype(np.float64) * (1.0 + mean_factor * u), flat.edge_mean).astype(np.float32)
    std = np.where(upper, flat.edge_std.astype(np.float64) * (1.0 + std_factor * v), flat.edge_std).astype(np.float32)
    return dataclasses.replace(flat, edge_mean=np.ascontiguousarray(mean), edge_std=np.ascontiguousarray(std))


A3_SETS = (("model_6oim_like", "set_6oim_c8", 64), ("model_6oim_like", "set_6oim_c64", 8), ("model_large110", "set_l110_c8", 4))


@functools.lru_cache(maxsize=None)
def a3_cases():
    """The golden models made asymmetric, against the first golden ligands of their sets (the 110-node model: node sets of two words)."""
    from pharmaconet_amd import PackedLibrary

    out = []
    for model, name, take in A3_SETS:
        flat = asym_scaled(golden_flat(model))
        _, lib, weights, _ = load_golden(name)
        assert weights is None
        lib = PackedLibrary.from_records([lib.record(i) for i in range(take)])
        out.append(Case(f"a3_{name}", flat, lib, oracle_scores(flat, lib)))
    return tuple(out)


# ------------------------------------------------------------------------------------------------ B: two-window cells
B1_CELL = 32  # [4.0, 4.125) of `gap_in_cell`


def gap_edges(flat):
    """wlo and whi of edges (0, 1) and (0, 2) of a `gap_model`, ascending."""
    t = host_tables(flat)
    return sorted(float(t[k][e]) for k in ("wlo", "whi") for e in (1, 2))


def _gap_case(name, flat, sweep, aim):
    sweep = np.unique(np.asarray(sweep, dtype=np.float32))  # ascending
    out = []
    for C in (1, 64):
        lib, dist, _ = library(pair_record, [(1, 1)], in_records(sweep, C))
        out.append(Case(f"{name}_c{C}", flat, lib, oracle_scores(flat, lib), dist, aim))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def b1_cases():
    """`gap_in_cell`, the subset pair ({0}, {1, 2}): every float within 32 ulps of each of the four window ends, 2048 evenly spaced floats
    of cell 32, the last float of cell 31 and the first of cell 33. (C = 1 case, C = 64 case); aim = (first, last float of the cell)."""
    flat = HAND_MODELS["gap_in_cell"]()
    h = F32(0.125)
    x0, x1 = F32(B1_CELL) * h, F32(B1_CELL + 1) * h
    sweep = [around(e, 32) for e in gap_edges(flat)] + [x0 + np.arange(2048, dtype=np.float32) * (h / F32(2048)), [down(x0), x1]]
    return _gap_case("b1", flat, np.concatenate(sweep), (x0, down(x1)))


@functools.lru_cache(maxsize=None)
def b2_cases():
    """`gap_on_cell_edge`: every float within 32 ulps of 4.0 and of each window end (the first window's last float is the last of its cell)."""
    flat = HAND_MODELS["gap_on_cell_edge"]()
    sweep = [around(e, 32) for e in gap_edges(flat)] + [around(4.0, 32)]
    return _gap_case("b2", flat, np.concatenate(sweep), None)


def complex_cells(flat):
    """(sa, sb, cell) of every cell of the model's functions that holds two pass windows: the NaN entries of `win`."""
    t = host_tables(flat)
    pairs = function_pairs(t)
    return t, [(pairs[fid][0], pairs[fid][1], int(i)) for fid, i in np.argwhere(np.isnan(t["win"][:, :, 0]))]


def masks_of(t, sid, K):
    """(cluster, mask) pairs that select subset `sid`."""
    return [(a, mask) for a in range(K) for mask in range(1, 128) if int(t["sidtab"][a * 128 + mask]) == sid]


@functools.lru_cache(maxsize=None)
def b3_cases():
    """The complex cells of `model_6oim_like`: per cell a (C = 1 case, C = 64 case) pair of the model reduced to two clusters that hold the
    cell's two subsets, against ligands of two one-node clusters whose masks select them - the pair entry of (cluster 0, cluster 1) is the one
    item of the cell's function. 256 evenly spaced floats of the cell and 8 ulps either side of every break point inside it.
    aim = (sa, sb, cell, ca, cb, m0, m1, reached): `reached` where the oracle's C = 1 scores hold a zero and a non-zero inside the cell, so that
    the majority count decides a score there (the other assignment of the two ligand clusters, or the centre prefilter, may hide it)."""
    full = golden_flat("model_6oim_like")
    t, cells = complex_cells(full)
    nm, h = full.num_nodes, F32(t["h"])
    out = []
    for sa, sb, i in cells:
        A, B = subset_nodes(t, sa), subset_nodes(t, sb)
        x0, x1 = F32(i) * h, F32(i + 1) * h
        e = (A[:, None] * nm + B[None, :]).reshape(-1)
        e = e[t["wok"][e] != 0]
        brk = np.concatenate([t["wlo"][e], up(t["whi"][e])]).astype(np.float32)
        brk = np.unique(brk[(brk > x0) & (brk < x1)])
        sweep = np.concatenate([x0 + np.arange(256, dtype=np.float32) * (h / F32(256))] + [around(b, 8) for b in brk])
        sweep = np.unique(sweep[(sweep >= x0) & (sweep < x1)])
        # the first choice of clusters and masks under which the cell's majority count decides a score (else the first of all)
        choices = [(ca, m0, cb, m1) for ca, m0 in masks_of(t, sa, full.num_clusters) for cb, m1 in masks_of(t, sb, full.num_clusters) if ca != cb]
        tried = []
        for ca, m0, cb, m1 in choices:
            flat = _two_cluster_model(full, ca, cb)
            lib, dist, _ = library(pair_record, [(m0, m1)], in_records(sweep, 1))
            ref = oracle_scores(flat, lib)
            tried.append((bool((ref == 0).any() and (ref > 0).any()), ca, m0, cb, m1, flat, lib, dist, ref))
            if tried[-1][0]:
                break
        decided, ca, m0, cb, m1, flat, lib, dist, ref = next((x for x in tried if x[0]), tried[0])
        lib64, dist64, _ = library(pair_record, [(m0, m1)], in_records(sweep, 64))
        pair = [[f"b3_s{sa}_s{sb}_cell{i}_c1", flat, lib, ref, dist], [f"b3_s{sa}_s{sb}_cell{i}_c64", flat, lib64, oracle_scores(flat, lib64), dist64]]
        aim = (sa, sb, i, ca, cb, m0, m1, decided)
        out.append(tuple(Case(*p, aim) for p in pair))
    return tuple(out)


# ------------------------------------------------------------------------------------------------ C: window ends on the golden models
C_MODELS = ("model_6oim_like", "model_stress64")
C_SINGLE, C_MULTI, C_ULPS, C_MAX_DRAWS = 32, 16, 4, 20000


@dataclasses.dataclass(frozen=True, eq=False)
class EdgeFunction:
    """One function of C: model clusters (a, b), node subsets A of a and B of b with their masks, and per edge (m, n) of A x B its window
    (wlo, whi). `case`: the model reduced to (a, b) against C = 1 ligands, in edge order the floats round wlo, then those round whi."""

    a: int
    b: int
    A: tuple
    B: tuple
    windows: tuple
    case: Case


def window_ends(fn):
    """Per window end of the function ([edges, 2]: wlo, whi): `decided` - the oracle's score is non-zero from wlo up and exactly zero below
    it, or non-zero up to whi and exactly zero above - and `constant` - non-zero at all the swept floats round the end, or zero at all."""
    d, alive = fn.case.dist[:, 0], fn.case.ref > 0
    n = 2 * C_ULPS + 1
    decided, constant = np.zeros((len(fn.windows), 2), dtype=bool), np.zeros((len(fn.windows), 2), dtype=bool)
    for k, (lo, hi) in enumerate(fn.windows):
        for side, inside in ((0, lambda x: x >= lo), (1, lambda x: x <= hi)):
            at = slice((2 * k + side) * n, (2 * k + side + 1) * n)
            decided[k, side] = np.array_equal(alive[at], inside(d[at]))
            constant[k, side] = alive[at].all() or not alive[at].any()
    return decided, constant


def kept(fn):
    """A function of one node pair: both ends of its window decided. Of more: see `c_functions`."""
    decided, constant = window_ends(fn)
    if len(fn.windows) == 1:
        return bool(decided.all())
    return bool(decided.sum() >= 2 and (decided | constant).all())


@functools.lru_cache(maxsize=None)
def c_functions(model):
    """From default_rng(5): C_SINGLE functions of one node pair and C_MULTI of more, between two different clusters of the golden model.
    With one pair the majority test is the edge's window, and both its ends must be decided by a float: a function where the other assignment
    of the two ligand clusters or the centre prefilter keeps the score alive or dead on both sides is dropped and the next one drawn. With
    more pairs the majority turns at some window ends only - at wlo where exactly one pass was missing, at whi where none was to spare - and
    neither golden model has a function of several pairs that turns at every end of every edge (0 of 1080 and 0 of 1292 between two
    clusters; the most are 6 ends of 15 pairs). Kept are those with at least two decided ends whose other ends leave the score as it is:
    every end of every edge is swept, each is decided or constant, and the majority count is what tells them apart."""
    from test_model_tables_cpu import passes

    full = golden_flat(model)
    t = host_tables(full)
    nm = full.num_nodes
    mean, std = full.edge_mean.reshape(-1), full.edge_std.reshape(-1)
    subsets = [list(_subsets(full, a).items()) for a in range(full.num_clusters)]
    rng = np.random.default_rng(5)
    single, multi = [], []
    for _ in range(C_MAX_DRAWS):
        if len(single) == C_SINGLE and len(multi) == C_MULTI:
            break
        a, b = (int(x) for x in rng.choice(full.num_clusters, 2, replace=False))
        (A, m0), (B, m1) = subsets[a][rng.integers(len(subsets[a]))], subsets[b][rng.integers(len(subsets[b]))]
        bucket, want = (single, C_SINGLE) if len(A) * len(B) == 1 else (multi, C_MULTI)
        e = np.array([m * nm + n for m, n in itertools.product(A, B)])
        if len(bucket) == want or not (t["wok"][e].all() and (t["wlo"][e] > 0).all()):
            continue
        lo, hi = t["wlo"][e], t["whi"][e]
        if len(e) > 1:  # (the oracle is asked only where the host's windows say that two ends turn the majority)
            majority = lambda d: 2 * passes(d, mean[e], std[e]).sum(axis=1) >= len(e)
            if int((majority(lo) & ~majority(down(lo))).sum() + (majority(hi) & ~majority(up(hi))).sum()) < 2:
                continue
        windows = tuple((F32(x), F32(y)) for x, y in zip(lo, hi))
        sweep = np.concatenate([around(x, C_ULPS) for w in windows for x in w])
        flat = _two_cluster_model(full, a, b)
        lib, dist, _ = library(pair_record, [(m0, m1)], in_records(sweep, 1))
        fn = EdgeFunction(a, b, A, B, windows, Case(f"c_{model}_{a}_{b}_{m0}_{m1}", flat, lib, oracle_scores(flat, lib), dist, (m0, m1)))
        if kept(fn):
            bucket.append(fn)
    return tuple(single), tuple(multi)


# ------------------------------------------------------------------------------------------------ D: the header's limits
D_NODES, D_CLUSTERS, D_REACH = 256, 128, (0, 63, 64, 127)


@functools.lru_cache(maxsize=None)
def d_model():
    """`model_6oim_like` tiled as test_gpu_hotspots.enlarged tiles it - node m + t * 37 is copy t of node m, its edges shifted by a few
    hundredths of an Angstrom per copy - and cut to 256 nodes; cluster k is copy k // 11 of cluster k % 11 with its members spread over the
    node copies, 128 of them; the last cluster holds node 255 and node 29 (word 0), both Anion."""
    base = golden_flat("model_6oim_like")
    nm, K0 = base.num_nodes, base.num_clusters
    copies = -(-D_NODES // nm)
    src, t = np.arange(D_NODES) % nm, np.arange(D_NODES) // nm
    shift = (0.03 * ((t[:, None] + t[None, :]) % 4)).astype(np.float32)
    members = cluster_lists(base)
    clusters = []
    for k in range(D_CLUSTERS):
        a, r = k % K0, k // K0
        nodes = {m + ((m + a + r) % copies) * nm for m in members[a]}
        clusters.append(sorted(n if n < D_NODES else n - nm for n in nodes))
    clusters[-1] = [29, D_NODES - 1]
    which = np.arange(D_CLUSTERS) % K0
    flat = hand_model(base.node_type[src], base.edge_mean[np.ix_(src, src)] + shift, base.edge_std[np.ix_(src, src)], clusters,
                      centers=np.asarray(base.cluster_center)[which], sizes=np.asarray(base.cluster_size)[which])
    assert flat.num_nodes == D_NODES and flat.num_clusters == D_CLUSTERS
    return flat


@functools.lru_cache(maxsize=None)
def d_case():
    """16 two-cluster ligands whose masks are the type masks of clusters 0, 63, 64 and 127: the 12 ordered pairs of them as one-node
    clusters at a distance where the aimed subsets' item passes, and 4 more with two nodes per cluster."""
    from pharmaconet_amd import PackedLibrary

    flat = d_model()
    lists = cluster_lists(flat)
    recs = []

    def place(a, b):
        d = _pin(flat, lists[a], lists[b])
        return float(d) if d is not None else float(flat.edge_mean[lists[a][0], lists[b][0]])

    for a, b in itertools.permutations(D_REACH, 2):
        recs.append(pair_record(int(flat.cluster_typemask[a]), int(flat.cluster_typemask[b]), np.array([place(a, b)], dtype=np.float32)))
    for a, b in ((0, 127), (127, 63), (63, 64), (64, 0)):
        d = place(a, b)
        xyz = np.zeros((4, 3, 2), dtype=np.float32)
        xyz[1, 1, :] = 1.5
        xyz[2, 0, :], xyz[3, 0, :], xyz[3, 1, :] = (d, d + 0.05), (d, d - 0.05), 1.5
        recs.append(_record([int(flat.cluster_typemask[a])] * 2, [int(flat.cluster_typemask[b])] * 2, xyz))
    lib = PackedLibrary.from_records(recs)
    return Case("d_limits", flat, lib, oracle_scores(flat, lib))
