"""Host-side helpers of bench.py (no GPU): the cores a process is really granted, and the tiling of a feature batch for the end-to-end pipeline leg."""

import os

import numpy as np


def test_host_cores_respects_affinity_and_cgroup_quota():
    import bench

    cores, info = bench.host_cores()
    assert 1 <= cores <= (os.cpu_count() or 1)
    assert info["usable_cores"] == cores and info["affinity"] >= cores
    if info["cgroup_cpu_max"] and info["cgroup_cpu_max"].split()[0] not in ("max", "-1"):
        quota, period = (int(x) for x in info["cgroup_cpu_max"].split())
        if quota > 0:
            assert cores <= max(1, int(quota / period + 0.5))


def test_tile_features_keeps_the_topologies_and_moves_the_geometry():
    import bench
    from pharmaconet_amd.library import flatten_features, pack_features_native
    from tools.synthetic import synthetic_library

    mols = []
    base = synthetic_library(48, num_conformers=8, seed=5, conformer_noise=0.0, molecules_out=mols)
    flat = flatten_features(mols)
    tiled = bench.tile_features(flat, 4, np.random.default_rng(1))
    lib, status = pack_features_native(tiled, threads=2)
    assert len(lib) == 4 * len(base) and status.sum() == 0
    hb = base.headers()
    for r in range(4):
        np.testing.assert_array_equal(lib.headers()[r * len(base) : (r + 1) * len(base)], hb)
    n, _, k = base.header(3)
    head = 8 + n + k
    assert lib.record(3)[:head] == base.record(3)[:head] == lib.record(3 + len(base))[:head]  # same types and clusters ...
    assert lib.record(3) != lib.record(3 + len(base)) != base.record(3)  # ... other coordinates in every copy


def test_reference_rate_file_is_what_bench_quotes():
    import bench

    ref = bench.reference_rate()
    assert ref is not None and ref["kind"] == "reference" and ref["cores"] == 1 and ref["value"] > 0
    for row in ref["sets"].values():
        assert row["ligand_conformers"] == 8 * row["ligands"]


def _fake_results(n, pockets, k, seed):
    """What bench.py's step() returns, on the CPU: per pocket (result with scores / status, (top-k scores, top-k indices))."""
    from types import SimpleNamespace

    import torch

    rng = np.random.default_rng(seed)
    out = []
    for _ in range(pockets):
        scores = torch.from_numpy(rng.random(n, dtype=np.float32))
        status = torch.from_numpy(rng.integers(0, 2, n).astype(np.int32))
        top = torch.topk(scores, k)
        out.append((SimpleNamespace(scores=scores, status=status), (top.values, top.indices.to(torch.int64) + 10**9)))
    return out


def test_dump_outputs_writes_every_array_in_float(tmp_path):
    import bench

    results = _fake_results(5000, 2, 7, seed=1)
    written = bench.dump_outputs(tmp_path, results)
    assert sorted(written) == sorted(f"{a}_pocket{p:02d}.npy" for a in ("scores", "status", "topk_scores", "topk_indices") for p in (0, 1))
    for p, (res, top) in enumerate(results):
        s = np.load(tmp_path / f"scores_pocket{p:02d}.npy")
        assert s.dtype == np.float32 and np.array_equal(s, res.scores.numpy())
        st = np.load(tmp_path / f"status_pocket{p:02d}.npy")
        assert st.dtype == np.float32 and np.array_equal(st, res.status.numpy())
        ti = np.load(tmp_path / f"topk_indices_pocket{p:02d}.npy")
        assert ti.dtype == np.float64 and ti.astype(np.int64).tolist() == top[1].tolist()


def test_dump_outputs_keeps_a_fixed_sample_within_the_budget(tmp_path):
    import bench

    n, budget = 100_000, 200_000
    results = _fake_results(n, 1, 5, seed=2)
    bench.dump_outputs(tmp_path / "a", results, rank=1, world=2, budget=budget)
    bench.dump_outputs(tmp_path / "b", results, rank=1, world=2, budget=budget)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(f"{a}_rank1.npy" for a in ("ligand_index", "scores", "status", "topk_scores", "topk_indices"))
    assert sum((tmp_path / "a" / f).stat().st_size for f in files) <= budget // 2  # (this rank's share of the budget)
    index = np.load(tmp_path / "a" / "ligand_index_rank1.npy")
    assert index.dtype == np.float64 and 0 < len(index) < n and np.all(np.diff(index) > 0)
    np.testing.assert_array_equal(index, np.load(tmp_path / "b" / "ligand_index_rank1.npy"))
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "scores_rank1.npy"), results[0][0].scores.numpy()[index.astype(np.int64)])
