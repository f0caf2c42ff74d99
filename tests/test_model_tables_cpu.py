"""The host arithmetic behind a device model (csrc/pmx_model_tables.cpp), without a GPU: every table `pmx_model_create` uploads, read through
the private `pmxt_*` hook of the host-only library and held to a NumPy float32 restatement of the reference's test
`abs((d - mean) / std) < 2` (match_utils.py:55-61), and to the bytes the code gave before it moved out of pmx_api.hip."""

import ctypes
import hashlib
import json
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO

F32 = np.float32
INF = F32(np.inf)
GOLDEN_MODELS = ("model_6oim_like", "model_clustered21", "model_stress64", "model_large110")


# ------------------------------------------------------------------------------------------ the hook
class TablesView(ctypes.Structure):
    """pmxt_tables_view (csrc/pmx_model_tables.h)."""

    _fields_ = (
        [(n, ctypes.c_int32) for n in ("Nm", "K", "symmetric")]
        + [(n, ctypes.c_uint32) for n in ("NS", "NF", "ncell")]
        + [("h", ctypes.c_float), ("n_complex_cells", ctypes.c_uint64)]
        + [(n, ctypes.c_void_p) for n in ("edge", "cpair", "cwin", "win", "wlo", "whi", "node_type", "sub_nodes", "wok", "tclus", "sidtab", "sub_off")]
        + [(n, ctypes.c_uint64) for n in ("n_edge", "n_cpair", "n_cwin", "n_win", "n_node_type", "n_sub_nodes", "n_tclus", "n_sidtab", "n_sub_off")]
    )


@pytest.fixture(scope="module")
def hook():
    import __graft_entry__ as entry

    entry.build()
    from pharmaconet_amd import _ffi

    lib = ctypes.CDLL(str(_ffi.LIB_PATH.with_name("libpmx_pack.so")))
    lib.pmxt_tables_create.argtypes = [ctypes.POINTER(_ffi.ModelDesc), ctypes.POINTER(ctypes.c_void_p)]
    lib.pmxt_tables_view_get.argtypes = [ctypes.c_void_p, ctypes.POINTER(TablesView)]
    lib.pmxt_tables_destroy.argtypes = [ctypes.c_void_p]
    lib.pmx_last_error.restype = ctypes.c_char_p
    return lib


def make_desc(flat):
    """(pmx_model_desc, the arrays it points into) of a FlatModel, as engine._ModelHandle makes it."""
    from pharmaconet_amd import _ffi

    keep = [
        np.ascontiguousarray(flat.node_type, dtype=np.uint8),
        np.ascontiguousarray(flat.edge_mean, dtype=np.float32),
        np.ascontiguousarray(flat.edge_std, dtype=np.float32),
        np.ascontiguousarray(flat.cluster_nodes, dtype=np.uint64),
        np.ascontiguousarray(flat.cluster_typemask, dtype=np.uint8),
        np.ascontiguousarray(flat.cluster_center, dtype=np.float64),
        np.ascontiguousarray(flat.cluster_size, dtype=np.float64),
    ]
    return _ffi.ModelDesc(flat.num_nodes, flat.num_clusters, *(a.ctypes.data for a in keep)), keep


def build_tables(lib, flat):
    """Every array of ModelTables as a NumPy copy, and its scalars."""
    desc, keep = make_desc(flat)
    handle = ctypes.c_void_p()
    rc = lib.pmxt_tables_create(ctypes.byref(desc), ctypes.byref(handle))
    assert rc == 0, lib.pmx_last_error()
    try:
        v = TablesView()
        assert lib.pmxt_tables_view_get(handle, ctypes.byref(v)) == 0

        def arr(ptr, n, dtype, per=1):
            n = int(n) * per
            if n == 0:
                return np.zeros(0, dtype)
            return np.frombuffer(ctypes.string_at(ptr, n * np.dtype(dtype).itemsize), dtype=dtype).copy()

        nm2 = v.Nm * v.Nm
        assert v.n_edge == nm2 and v.n_cpair == v.n_cwin == v.K * v.K and v.n_win == v.NF * v.ncell
        assert v.n_node_type == 256 and v.n_tclus == 256 and v.n_sidtab == max(v.K, 1) * 128 and v.n_sub_off == v.NS + 1
        t = dict(
            Nm=v.Nm, K=v.K, symmetric=v.symmetric, NS=v.NS, NF=v.NF, ncell=v.ncell, h=float(v.h), n_complex_cells=v.n_complex_cells,
            edge=arr(v.edge, v.n_edge, np.float32, 4).reshape(-1, 4),
            cpair=arr(v.cpair, v.n_cpair, np.float32, 2).reshape(-1, 2),
            cwin=arr(v.cwin, v.n_cwin, np.float32, 2).reshape(-1, 2),
            win=arr(v.win, v.n_win, np.float32, 2).reshape(v.NF, v.ncell, 2),
            wlo=arr(v.wlo, nm2, np.float32), whi=arr(v.whi, nm2, np.float32), wok=arr(v.wok, nm2, np.uint8),
            node_type=arr(v.node_type, v.n_node_type, np.uint8), sub_nodes=arr(v.sub_nodes, v.n_sub_nodes, np.uint8),
            tclus=arr(v.tclus, v.n_tclus, np.uint64), sidtab=arr(v.sidtab, v.n_sidtab, np.uint16), sub_off=arr(v.sub_off, v.n_sub_off, np.uint32),
        )
    finally:
        lib.pmxt_tables_destroy(handle)
    return t


# ------------------------------------------------------------------------------------------ models
def hand_model(node_type, mean, std, clusters, centers=None, sizes=None):
    """A FlatModel from node types, [Nm, Nm] means and stds and the clusters' node lists (a cluster's type mask: its nodes' types)."""
    from pharmaconet_amd.pharmacophore_model import FlatModel, _node_masks

    nm, k = len(node_type), len(clusters)
    node_type = np.array(node_type, dtype=np.uint8)
    masks = [sum(1 << m for m in c) for c in clusters]
    return FlatModel(
        node_type=node_type,
        edge_mean=np.array(mean, dtype=np.float32).reshape(nm, nm),
        edge_std=np.array(std, dtype=np.float32).reshape(nm, nm),
        cluster_nodes=_node_masks(masks, nm) if k else np.zeros(0, np.uint64),
        cluster_typemask=np.array([np.bitwise_or.reduce([1 << int(node_type[m]) for m in c]) for c in clusters], dtype=np.uint8),
        cluster_center=np.array(centers if centers is not None else [[1.5 * a, 0.25 * a, -a] for a in range(k)], dtype=np.float64).reshape(k, 3),
        cluster_size=np.array(sizes if sizes is not None else [1.0 + 0.5 * a for a in range(k)], dtype=np.float64),
        cluster_type=("Hydrophobic",) * k,
    )


def gap_model(m1, m2):
    """Node 0 alone in cluster 0; nodes 1, 2 in cluster 1, at means m1 and m2 from node 0 (std 0.5: cells of 0.125). Half of two node pairs
    is one, so the pair of subsets ({0}, {1, 2}) passes inside either edge's window: two runs with a gap between them."""
    mean = [[0.0, m1, m2], [m1, 0.0, 2.0], [m2, 2.0, 0.0]]
    return hand_model([0, 0, 0], mean, np.full((3, 3), 0.5), [[0], [1, 2]])


HAND_MODELS = {
    "empty": lambda: hand_model([], [], [], []),
    "one_node": lambda: hand_model([3], [[0.0]], [[0.8]], [[0]]),
    "two_nodes_no_cluster": lambda: hand_model([0, 4], [[0.0, 4.0], [4.0, 0.0]], [[0.5, 0.7], [0.7, 0.5]], []),
    "asym3": lambda: hand_model(
        [0, 0, 4],
        [[0.0, 3.0, 5.5], [3.4, 0.0, 4.25], [6.0, 4.0, 0.0]],
        [[0.5, 0.6, 0.9], [0.7, 0.5, 0.55], [0.8, 0.6, 0.5]],
        [[0, 1], [2], [0, 2]],
    ),
    # windows (2.05, 4.05) and (4.07, 6.07): the gap lies inside the cell [4.0, 4.125), which therefore holds two runs
    "gap_in_cell": lambda: gap_model(3.05, 5.07),
    # windows [2, 4) and (4.02, 6.02): the first one ends with the last float of the cell [3.875, 4.0), so every cell holds one run
    "gap_on_cell_edge": lambda: gap_model(3.0, 5.02),
}

_cache = {}


def tables(lib, name):
    """(FlatModel, its tables): computed once per model and shared by the tests, which leave them unchanged."""
    if name not in _cache:
        if name in HAND_MODELS:
            flat = HAND_MODELS[name]()
        else:
            from pharmaconet_amd import PharmacophoreModel

            flat = PharmacophoreModel.load(GOLDEN / f"{name}.pm").flat
        _cache[name] = (flat, build_tables(lib, flat))
    return _cache[name]


ALL_MODELS = tuple(HAND_MODELS) + GOLDEN_MODELS


# ------------------------------------------------------------------------------------------ the reference predicate
def passes(d, mean, std):
    """abs((d - mean) / std) < 2 in float32, as match_utils.py:55-57 evaluates it: d [P] against edges [M] -> [P, M]."""
    d = np.asarray(d, dtype=F32).reshape(-1, 1)
    with np.errstate(over="ignore"):  # (the largest float, over a std below one)
        return np.abs((d - np.asarray(mean, F32).reshape(1, -1)) / np.asarray(std, F32).reshape(1, -1)) < F32(2)


def up(x):
    return np.nextafter(np.asarray(x, F32), INF)


def down(x):
    return np.nextafter(np.asarray(x, F32), -INF)


def subset_nodes(t, s):
    return t["sub_nodes"][t["sub_off"][s] : t["sub_off"][s + 1]].astype(int)


def cluster_lists(flat):
    cn = np.asarray(flat.cluster_nodes, dtype=np.uint64).reshape(flat.num_clusters, max(1, (flat.num_nodes + 63) // 64))
    return [[m for m in range(flat.num_nodes) if int(words[m // 64]) >> (m % 64) & 1] for words in cn]


# ------------------------------------------------------------------------------------------ edges
@pytest.mark.parametrize("name", ALL_MODELS)
def test_edge_windows_are_the_predicate(hook, name):
    flat, t = tables(hook, name)
    mean, std = flat.edge_mean.reshape(-1).astype(F32), flat.edge_std.reshape(-1).astype(F32)
    assert np.array_equal(t["edge"][:, 0], mean) and np.array_equal(t["edge"][:, 3], std)
    assert np.array_equal(t["edge"][:, 1], (np.sqrt(0.5 * 1.4426950408889634074) / std.astype(np.float64)).astype(F32))
    # T: the largest float with fl(T / std) < 2
    T = t["edge"][:, 2]
    assert np.all(T / std < F32(2)) and np.all(up(T) / std >= F32(2))
    if mean.size == 0:
        return
    ok = t["wok"] != 0
    lo, hi = t["wlo"], t["whi"]
    diag = lambda d: np.abs((np.asarray(d, F32) - mean) / std) < F32(2)  # one distance per edge
    assert np.all(diag(lo)[ok]) and np.all(diag(hi)[ok])
    assert not np.any(diag(up(hi))[ok])
    below = ok & (lo > 0)
    assert not np.any(diag(down(lo))[below])
    assert np.all(lo[ok] >= 0) and np.all(lo[ok] <= hi[ok])
    rng = np.random.default_rng(1)
    # random floats around the window, and the floats next to its ends
    for _ in range(64):
        d = np.maximum(mean + std * rng.uniform(-3.0, 3.0, mean.size).astype(F32), F32(0)).astype(F32)
        assert np.array_equal(diag(d), ok & (lo <= d) & (d <= hi))
    for end in (lo, hi):
        d = np.where(ok, end, F32(0)).astype(F32)
        for step in (up, down):
            x = d.copy()
            for _ in range(4):
                x = np.maximum(step(x), F32(0)).astype(F32)
                assert np.array_equal(diag(x), ok & (lo <= x) & (x <= hi))
    assert not np.any(diag(np.zeros_like(mean))[~ok])  # (an edge without a window passes nowhere; 0 is where it would start)


# ------------------------------------------------------------------------------------------ subsets, clusters
@pytest.mark.parametrize("name", ALL_MODELS)
def test_node_subsets(hook, name):
    flat, t = tables(hook, name)
    clusters = cluster_lists(flat)
    assert t["Nm"] == flat.num_nodes and t["K"] == flat.num_clusters
    assert np.array_equal(t["node_type"][: flat.num_nodes], flat.node_type) and not t["node_type"][flat.num_nodes :].any()
    assert t["sub_off"][0] == 0 and t["sub_off"][1] == 0  # subset 0 is the empty one
    seen = {}
    for a, nodes in enumerate(clusters):
        for mask in range(128):
            want = [m for m in nodes if mask >> int(flat.node_type[m]) & 1]
            sid = int(t["sidtab"][a * 128 + mask])
            assert sid < t["NS"]
            assert subset_nodes(t, sid).tolist() == want, (a, mask)
            assert (sid == 0) == (not want)
            seen[sid] = tuple(want)
    assert len(set(seen.values())) == len(seen)  # one id per distinct set
    assert t["NS"] == 1 + len([s for s in seen if s != 0])
    if not clusters:
        assert not t["sidtab"].any()
    # tclus: the model clusters that share a type with a ligand type mask
    for mask in range(128):
        want = sum(1 << a for a in range(flat.num_clusters) if int(flat.cluster_typemask[a]) & mask)
        assert int(t["tclus"][2 * mask]) | int(t["tclus"][2 * mask + 1]) << 64 == want
    sym = bool(np.array_equal(flat.edge_mean, flat.edge_mean.T) and np.array_equal(flat.edge_std, flat.edge_std.T))
    assert t["symmetric"] == int(sym)
    assert t["NF"] == (t["NS"] * (t["NS"] + 1) // 2 if sym else t["NS"] * t["NS"])


@pytest.mark.parametrize("name", ALL_MODELS)
def test_cluster_pairs(hook, name):
    flat, t = tables(hook, name)
    K, Nm = flat.num_clusters, flat.num_nodes
    clusters = cluster_lists(flat)
    c = np.asarray(flat.cluster_center, np.float64).reshape(K, 3)
    for a in range(K):
        for b in range(K):
            dx, dy, dz = c[a] - c[b]
            want = (F32(np.sqrt(dx * dx + dy * dy + dz * dz)), F32(flat.cluster_size[a] + flat.cluster_size[b]))
            assert tuple(t["cpair"][a * K + b]) == want
            e = np.array([m * Nm + n for m in clusters[a] for n in clusters[b]], dtype=int)
            e = e[t["wok"][e] != 0] if e.size else e
            hull = (t["wlo"][e].min(), t["whi"][e].max()) if e.size else (INF, -INF)
            assert tuple(t["cwin"][a * K + b]) == hull


# ------------------------------------------------------------------------------------------ cells
def check_cell(flat, t, sa, sb, i, rng):
    """One cell of the function of subsets (sa, sb), decided exactly. The majority `2 * passes >= pairs` can change only at an edge window's
    first float or at the float after its last, so the predicate at those floats and at the cell's first float gives every run of the cell;
    random floats inside the cell must agree with the piece they fall in. Returns the number of passing runs."""
    tri = t["symmetric"] != 0
    fid = sa * (sa + 1) // 2 + sb if tri else sa * t["NS"] + sb
    lo, hi = t["win"][fid, i]
    A, B = subset_nodes(t, sa), subset_nodes(t, sb)
    if A.size == 0 or B.size == 0:  # no item: never a fail
        assert lo == -INF and hi == INF
        return 1
    h, Nm = F32(t["h"]), flat.num_nodes
    x0 = F32(i) * h
    x1 = INF if i + 1 == t["ncell"] else F32(i + 1) * h
    e = (A[:, None] * Nm + B[None, :]).reshape(-1)
    mean, std = flat.edge_mean.reshape(-1)[e], flat.edge_std.reshape(-1)[e]
    majority = lambda d: 2 * passes(d, mean, std).sum(axis=1) >= e.size
    ok = t["wok"][e] != 0
    brk = np.concatenate([[x0], t["wlo"][e][ok], up(t["whi"][e][ok])]).astype(F32)
    brk = np.unique(brk[(brk >= x0) & (brk < x1)])  # ascending; brk[0] == x0
    ends = np.append(down(brk[1:]), down(x1)).astype(F32)  # last float of every piece (of the last cell's: the largest float)
    piece_ok = majority(brk)
    assert np.array_equal(majority(ends), piece_ok)  # (a piece is constant: its two ends agree)
    span = float(x1 - x0) if np.isfinite(x1) else 4.0 * float(h)
    d = (x0 + rng.uniform(0.0, span, 24).astype(F32)).astype(F32)
    d = d[(d >= x0) & (d < x1)]
    assert np.array_equal(majority(d), piece_ok[np.searchsorted(brk, d, side="right") - 1])
    runs = int(piece_ok[0]) + int(np.sum(piece_ok[1:] & ~piece_ok[:-1]))
    if np.isnan(lo):
        assert np.isnan(hi) and runs >= 2, (sa, sb, i, runs)
    else:
        assert lo <= hi
        inside = (lo <= brk) & (ends <= hi)
        outside = (hi < brk) | (ends < lo)
        assert np.all(np.where(piece_ok, inside, outside)), (sa, sb, i, lo, hi, brk, piece_ok)
        assert np.array_equal(majority(d), (lo <= d) & (d <= hi))
        assert runs <= 1
    return runs


def function_pairs(t):
    NS = t["NS"]
    return [(sa, sb) for sa in range(NS) for sb in range(sa + 1 if t["symmetric"] else NS)]


@pytest.mark.parametrize("name", tuple(HAND_MODELS))
def test_every_cell_of_the_small_models(hook, name):
    flat, t = tables(hook, name)
    rng = np.random.default_rng(2)
    pairs = function_pairs(t)
    assert len(pairs) == t["NF"]
    for sa, sb in pairs:
        for i in range(t["ncell"]):
            check_cell(flat, t, sa, sb, i, rng)
    assert t["n_complex_cells"] == int(np.isnan(t["win"][:, :, 0]).sum())
    if name == "asym3":  # (sa, sb) and (sb, sa) are functions of their own, each checked against its own node pairs above
        assert t["symmetric"] == 0 and t["NF"] == t["NS"] ** 2
    if name == "gap_in_cell":
        assert t["h"] == 0.125 and t["n_complex_cells"] >= 1
        s0, s12 = int(t["sidtab"][0 * 128 + 1]), int(t["sidtab"][1 * 128 + 1])
        assert subset_nodes(t, s0).tolist() == [0] and subset_nodes(t, s12).tolist() == [1, 2]
        sa, sb = max(s0, s12), min(s0, s12)
        assert np.isnan(t["win"][sa * (sa + 1) // 2 + sb, 32, 0])  # the cell [4.0, 4.125)
    if name == "gap_on_cell_edge":
        assert t["n_complex_cells"] == 0


@pytest.mark.parametrize("name", GOLDEN_MODELS)
def test_sampled_cells_of_the_golden_models(hook, name):
    flat, t = tables(hook, name)
    rng = np.random.default_rng(3)
    pairs = function_pairs(t)
    assert len(pairs) == t["NF"]
    for k in rng.choice(len(pairs), size=48, replace=False):
        sa, sb = pairs[k]
        for i in rng.choice(t["ncell"], size=24, replace=False):
            check_cell(flat, t, sa, sb, int(i), rng)
    # every cell that holds two windows, wherever it is
    nan = np.argwhere(np.isnan(t["win"][:, :, 0]))
    assert t["n_complex_cells"] == len(nan)
    for fid, i in nan:
        sa, sb = pairs[fid]
        assert check_cell(flat, t, sa, sb, int(i), rng) >= 2


# ------------------------------------------------------------------------------------------ byte pins
# What the code gave at the commit before it moved out of pmx_api.hip (g++ -O2 -ffp-contract=off): sha256[:16] of the raw little-endian arrays.
PINS = {
    "model_6oim_like": (37, 703, 107, 0.25, 9, "658a7b424ebc3c14", "11bdcf4724a24325", "08d233a9fde6acbe", "f4ed147c090fb7a8"),
    "model_clustered21": (23, 276, 111, 0.25, 0, "1adfd70c489527f4", "4015bb8006c1b0b6", "69d740bc296fbaee", "9d17a74cdabc5ece"),
    "model_stress64": (67, 2278, 153, 0.25, 0, "0aa48da683888763", "481829263a2e71df", "dc7c871c9eddf482", "d639a34212e871a6"),
    "model_large110": (108, 5886, 186, 0.25, 0, "a65703a344270f89", "17891832f687d2d3", "21446c9de3761c00", "e73ba0ac86d01a42"),
}


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).astype(a.dtype.newbyteorder("<"), copy=False).tobytes()).hexdigest()[:16]


@pytest.mark.parametrize("name", GOLDEN_MODELS)
def test_tables_are_the_bytes_of_the_code_they_came_from(hook, name):
    _, t = tables(hook, name)
    NS, NF, ncell, h, n_complex, sidtab, sub_off, sub_nodes, win = PINS[name]
    assert (t["NS"], t["NF"], t["ncell"], t["h"], t["n_complex_cells"]) == (NS, NF, ncell, h, n_complex)
    assert (digest(t["sidtab"]), digest(t["sub_off"]), digest(t["sub_nodes"]), digest(t["win"])) == (sidtab, sub_off, sub_nodes, win)
    recorded = json.loads((GOLDEN / "model_tables_digests.json").read_text())[name]
    for key in ("sidtab", "sub_off", "sub_nodes", "win", "edge", "tclus", "cpair", "cwin"):
        assert digest(t[key]) == recorded[key], key
    for key in ("NS", "NF", "ncell", "h", "n_complex_cells", "symmetric"):
        assert t[key] == recorded[key], key


# ------------------------------------------------------------------------------------------ errors
def test_invalid_models_are_refused_with_their_messages(hook):
    from pharmaconet_amd import _ffi

    def refused(desc, keep=None):
        handle = ctypes.c_void_p()
        assert hook.pmxt_tables_create(ctypes.byref(desc), ctypes.byref(handle)) == 1  # PMX_ERR_INVALID
        assert not handle.value
        return hook.pmx_last_error().decode()

    bad_std = HAND_MODELS["asym3"]()
    bad_std.edge_std[1, 2] = 0.0
    assert refused(*make_desc(bad_std)) == "edge 5 has distance_std 0"
    bad_std.edge_std[1, 2] = -1.0
    assert refused(*make_desc(bad_std)) == "edge 5 has distance_std -1"
    bad_type = HAND_MODELS["one_node"]()
    bad_type.node_type[0] = 7
    assert refused(*make_desc(bad_type)) == "node 0 has type id 7"
    assert refused(_ffi.ModelDesc(257, 0)) == "model has 257 nodes (max 256)"
    assert refused(_ffi.ModelDesc(0, 129)) == "model has 129 clusters (max 128)"
    assert hook.pmxt_tables_create(None, None) == 1 and b"null" in hook.pmx_last_error()


def test_packer_library_keeps_the_readers_messages():
    """libpmx_pack.so: an error of the SD reader leaves its message in pmx_last_error()."""
    import __graft_entry__ as entry

    entry.build()
    from pharmaconet_amd import _ffi

    lib = _ffi.load_packer()
    text = b"mol\n  prog\n\nnot a counts line\nM  END\n$$$$\n"
    assert lib.pmx_pack_features(None, 0, None, None, 0, None, None) == 1 and lib.pmx_last_error() == b"null argument"  # (what a stale message would be)
    n_rec, n_atoms = ctypes.c_uint64(), ctypes.c_uint64()
    per, z, xyz = np.zeros(4, np.int32), np.zeros(16, np.uint8), np.zeros(48, np.float32)
    rc = lib.pmx_sdf_heavy_atoms(text, len(text), 4, 4, 16, ctypes.byref(n_rec), ctypes.byref(n_atoms), per.ctypes.data, z.ctypes.data, xyz.ctypes.data)
    assert rc == 1
    assert b"pmx_sdf_heavy_atoms" in lib.pmx_last_error()


# ------------------------------------------------------------------------------------------ sanitizers
def test_tables_under_address_and_undefined_sanitizers(tmp_path):
    """tests/model_tables_main.cpp with the two host units under ASan and UBSan, as a program of its own."""
    csrc = REPO / "pharmaconet_amd" / "csrc"
    exe = tmp_path / "model_tables_main"
    cmd = ["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", f"-I{REPO / 'include'}", f"-I{csrc}",
           str(REPO / "tests" / "model_tables_main.cpp"), str(csrc / "pmx_model_tables.cpp"), str(csrc / "pmx_error.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    sys.stdout.write(run.stdout)
    assert run.returncode == 0, run.stderr[-2000:]
