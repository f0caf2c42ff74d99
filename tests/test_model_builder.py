"""`PharmacophoreModel.create` / `model_builder.build_model_state` against the reference's own `create`
(SURVEY.md section 8, row f3). Fixtures: tests/golden/make_golden_create.py ran the reference's
`PharmacophoreModel.create` (`pharmacophore_model.py:108-149`, `utils/density_map.py`) on synthetic hotspot
density maps (several components per map, touching blobs, specks under the 8-voxel floor) and saved its state."""

import contextlib
from pathlib import Path

import numpy as np
import pytest

from pharmaconet_amd import PharmacophoreModel
from pharmaconet_amd.model_builder import build_model_state, voxel_components

GOLDEN = Path(__file__).parent / "golden"
CASES = ["mixed24", "charged40", "crowded48"]


def load_inputs(name):
    z = np.load(GOLDEN / f"create_{name}_inputs.npz")
    infos = []
    for h in range(int(z["n"])):
        m = np.zeros((64, 64, 64), dtype=np.float32)
        idx = z[f"vox{h}"].astype(np.int64)
        m[tuple(idx.T)] = z[f"val{h}"]
        infos.append(dict(nci_type=str(z["kinds"][h]), hotspot_position=z["positions"][h], hotspot_score=float(z["scores"][h]),
                          point_map=m))
    return z["center"], infos


@contextlib.contextmanager
def only_the_device_search(monkeypatch, infos):
    """`build_model_state` has two ways back to the host loop - `device_search_agrees` and, in `create(device="auto")`, a caught
    RuntimeError - and either would leave a broken kernel unseen. Inside this block there is none: the self-check has passed, the
    host search raises, and on leaving it `voxel_components_device` has been called once, with all hotspot maps."""
    from pharmaconet_amd import model_builder

    assert model_builder.device_search_agrees(0) is True  # (runs the host search once per process: before it is taken away)
    calls = []
    device_search = model_builder.voxel_components_device

    def recorded(masks, device=0):
        calls.append((list(masks), device))
        return device_search(masks, device)

    def no_host_search(mask):
        raise AssertionError("build_model_state(device=0) fell back to the host search")

    with monkeypatch.context() as patch:
        patch.setattr(model_builder, "voxel_components_device", recorded)
        patch.setattr(model_builder, "voxel_components", no_host_search)
        yield
    assert len(calls) == 1 and calls[0][1] == 0
    assert len(calls[0][0]) == len(infos) and all(m is info["point_map"] for m, info in zip(calls[0][0], infos))


def _assert_state_equals_reference(name, device, monkeypatch=None):
    center, infos = load_inputs(name)
    want = PharmacophoreModel.load(GOLDEN / f"create_{name}.pm").__getstate__()
    with only_the_device_search(monkeypatch, infos) if device is not None else contextlib.nullcontext():
        got = build_model_state(want["pdbblock"], center, infos, device=device)
    assert got["pdbblock"] == want["pdbblock"]
    # nodes: numbering (component order), float32 centres, radii, edge maps and overlap lists - exact
    assert len(got["nodes"]) == len(want["nodes"])
    for g, w in zip(got["nodes"], want["nodes"]):
        assert g == w, (g["index"], g, w)
    # edges: index, end points, types, float mean / std - exact
    assert got["edges"] == want["edges"]
    assert got["node_dict"] == want["node_dict"]
    # clusters: kind order, member tuples (CPython set order), float32-mean centre and size - exact;
    # node_types is a tuple built from a set of strings in the reference (no defined order): compare as sets
    assert list(got["node_cluster_dict"]) == list(want["node_cluster_dict"])
    for kind in want["node_cluster_dict"]:
        gl, wl = got["node_cluster_dict"][kind], want["node_cluster_dict"][kind]
        assert len(gl) == len(wl), kind
        for g, w in zip(gl, wl):
            assert set(g.pop("node_types")) == set(w.pop("node_types"))
            assert g == w, (kind, g, w)


@pytest.mark.parametrize("name", CASES)
def test_state_equals_reference(name):
    _assert_state_equals_reference(name, None)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_state_equals_reference_with_the_searches_on_the_gpu(name, monkeypatch):
    """the voxel searches of `DensityMapGraph` on the device (`csrc/pmx_density.hip`: component labels +
    breadth-first member order per component), the seeds from CPython's own `set.pop()`: the same state as the reference's - and
    built by the device search, not by a fall-back to the host loop (`only_the_device_search`)."""
    _assert_state_equals_reference(name, 0, monkeypatch)


def synthetic_hotspots_24():
    """(center, hotspot infos) on a 24^3 grid: several components per map, blobs that touch, specks under the 8-voxel floor."""
    rng = np.random.default_rng(2424)
    g = np.stack(np.meshgrid(*[np.arange(24)] * 3, indexing="ij"), -1)
    kinds = ("Hydrophobic", "HBond_pdon", "PiStacking_P", "SaltBridge_pneg", "HBond_ldon", "Hydrophobic", "SaltBridge_lneg", "XBond")
    infos = []
    for h, kind in enumerate(kinds):
        m = np.zeros((24, 24, 24), dtype=np.float32)
        first = rng.integers(4, 20, size=3)
        balls = [(first, 2.6), (first + (3, 1, 0), 2.2)]  # two blobs that touch: one component
        balls += [(rng.integers(2, 22, size=3), rng.uniform(1.5, 3.2)) for _ in range(4 + h % 3)]
        for c, r in balls:
            inside = ((g - c) ** 2).sum(-1) <= r * r
            m[inside] = rng.uniform(0.05, 1.0, size=int(inside.sum())).astype(np.float32)
        m[rng.random(m.shape) < 0.002] = 0.3  # specks
        m[0, 0, 0] = m[23, 23, 23] = m[23, 23, 22] = 0.2
        infos.append(dict(nci_type=kind, hotspot_position=rng.uniform(-5, 5, size=3).astype(np.float32), hotspot_score=float(rng.uniform(0.3, 1.0)),
                          point_map=m))
    return np.array([1.5, -2.25, 3.0]), infos


def test_synthetic_hotspots_24_hold_what_they_are_named_for():
    _, infos = synthetic_hotspots_24()
    sizes = [[len(members) for members, _ in voxel_components(info["point_map"])] for info in infos]
    assert all(sum(s >= 8 for s in per_map) >= 2 for per_map in sizes)  # several components per map that become nodes
    assert all(any(s < 8 for s in per_map) for per_map in sizes)  # and specks that do not
    state = build_model_state(None, *synthetic_hotspots_24(), resolution=1.0, size=24)
    assert len(state["nodes"]) == sum(s >= 8 for per_map in sizes for s in per_map) >= 20
    assert sum(len(v) for v in state["node_cluster_dict"].values()) >= 4


@pytest.mark.gpu
def test_state_at_another_geometry_with_the_searches_on_the_gpu(monkeypatch):
    """A 24^3 grid at 1 A: the state built with the device search equals the one built with the host search, exactly."""
    center, infos = synthetic_hotspots_24()
    want = build_model_state("X", center, infos, resolution=1.0, size=24, device=None)
    with only_the_device_search(monkeypatch, infos):
        got = build_model_state("X", center, infos, resolution=1.0, size=24, device=0)
    assert len(want["nodes"]) >= 20
    for g, w in zip(got["nodes"], want["nodes"]):
        assert g == w, (g["index"], g, w)
    assert got == want


@pytest.mark.gpu
def test_device_member_lists_equal_the_host_search():
    """Every component of every map, voxel for voxel in discovery order, device against the host search (`voxel_components`, itself
    held to the reference by test_state_equals_reference): random blobs that touch through faces, edges and corners, specks, a
    solid 20^3 cube (8 000 voxels: wide frontiers), a thin diagonal line, voxels on the grid's faces, an empty map."""
    from pharmaconet_amd.model_builder import voxel_components_device

    rng = np.random.default_rng(20250523)
    masks = []
    for k in range(6):
        m = np.zeros((64, 64, 64), dtype=np.float32)
        for _ in range(12 + 6 * k):
            c = rng.integers(2, 62, size=3)
            r = rng.uniform(1.0, 5.5)
            g = np.stack(np.meshgrid(*[np.arange(64)] * 3, indexing="ij"), -1)
            inside = ((g - c) ** 2).sum(-1) <= r * r
            m[inside] = rng.uniform(0.05, 1.0, size=int(inside.sum())).astype(np.float32)
        m[rng.random(m.shape) < 0.0005] = 0.3  # specks
        masks.append(m)
    cube = np.zeros((64, 64, 64), dtype=np.float32)
    cube[5:25, 30:50, 40:60] = rng.uniform(0.1, 1.0, size=(20, 20, 20)).astype(np.float32)
    for i in range(40):
        cube[20 + i, 5 + i // 2, 63 - i] = 0.5  # a line that moves through corners, ending on a face
    cube[0, 0, 0] = cube[63, 63, 63] = cube[0, 63, 0] = 0.2
    masks.append(cube)
    masks.append(np.zeros((64, 64, 64), dtype=np.float32))
    got = voxel_components_device(masks, 0)
    n_comp = 0
    for m, comps in zip(masks, got):
        want = list(voxel_components(m))
        assert len(comps) == len(want)
        for (gm, gv), (wm, wv) in zip(comps, want):
            assert gm.tolist() == [list(p) for p in wm]
            assert gv.tolist() == wv
        n_comp += len(want)
    assert n_comp > 100 and max(len(w[0]) for w in voxel_components(cube)) >= 8000


def test_create_gives_a_scorable_model():
    center, infos = load_inputs("mixed24")
    made = PharmacophoreModel.create("X", center, infos)
    ref = PharmacophoreModel.load(GOLDEN / "create_mixed24.pm")
    a, b = made.flat, ref.flat
    assert a.num_nodes == b.num_nodes and a.num_clusters == b.num_clusters
    np.testing.assert_array_equal(a.edge_mean, b.edge_mean)
    np.testing.assert_array_equal(a.edge_std, b.edge_std)
    np.testing.assert_array_equal(a.cluster_nodes, b.cluster_nodes)
    np.testing.assert_array_equal(a.cluster_center, b.cluster_center)
    np.testing.assert_array_equal(a.cluster_size, b.cluster_size)


def test_components_are_26_connected_and_small_ones_are_dropped():
    m = np.zeros((64, 64, 64), dtype=np.float32)
    m[10:13, 10:13, 10:13] = 0.7          # 27 voxels
    m[13, 13, 13] = 0.6                    # touches the cube only through a corner: same component
    m[30, 30, 30] = m[31, 31, 30] = 0.9    # 2 voxels: a component, but below the floor of 8
    comps = sorted((len(v), sorted(v)[0]) for v, _ in voxel_components(m))
    assert comps == [(2, (30, 30, 30)), (28, (10, 10, 10))]
    st = build_model_state(None, (0.0, 0.0, 0.0), [dict(nci_type="Hydrophobic", hotspot_position=np.zeros(3, np.float32),
                                                      hotspot_score=1.0, point_map=m)])
    assert len(st["nodes"]) == 1 and len(st["edges"]) == 1
    assert st["nodes"][0]["overlapped_nodes"] == [0, 0]  # the self loop registers the node twice (density_map.py:247-249)
    assert [len(v) for v in st["node_cluster_dict"].values()] == [0, 0, 0, 0, 1, 0]


@pytest.mark.gpu
def test_device_search_checks_itself_against_the_interpreter():
    """`device_search_agrees`: the one-time comparison of the device search with the reference's own loop on a synthetic map passes
    on this interpreter (and is what `build_model_state` consults before it trusts the device with a model's state)."""
    from pharmaconet_amd import model_builder

    model_builder._DEVICE_SEARCH_OK.clear()
    assert model_builder.device_search_agrees(0) is True
    assert model_builder._DEVICE_SEARCH_OK == {0: True}
