#!/usr/bin/env python3
"""The hotspot row kernel and the fingerprint kernels alone, on the explained top of the bench's synthetic library.

    python tools/hotspots_bench.py [--ligands 1000000] [--rows 65536] [--out profiles/hotspots.json]

The 1 M-ligand synthetic library (8 conformers) is screened, its `--rows` best hits are explained, and on those rows - each at its best
conformer under its own key - HIP-event times of a warm call, best of three, of

    attribute   pmx_attribute: the yardstick, the steps pmx_hotspots shares with it
    hotspots    pmx_hotspots on the same rows: the same steps, G(u, v) per node pair, and the model-side step
    tanimoto    pmx_fingerprint_tanimoto of the rows' fingerprints against the first 4096 of them
    leaders     pmx_fingerprint_leaders at 0.7 over the rows in rank order

Prints one JSON line."""
import argparse
import ctypes
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def event_ms(torch, fn, reps=3):
    """Best of `reps` HIP-event times of fn(), after one warming call."""
    fn()
    torch.cuda.synchronize()
    best = 1e30
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        best = min(best, t0.elapsed_time(t1))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ligands", type=int, default=1_000_000)
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--against", type=int, default=4096, help="columns of the similarity block")
    ap.add_argument("--threshold", type=float, default=0.7)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import torch

    import bench
    from pharmaconet_amd import PharmacophoreModel, _ffi, engine

    model_file, n_conf, _, topologies, active, seed = bench.WORKLOADS["6oim"]
    model = PharmacophoreModel.load(bench.REPO / "tests" / "golden" / model_file)
    dev = torch.device("cuda", 0)
    dlib, offsets, data, _ = bench.build_library(model, args.ligands, n_conf, topologies, 0, dev, active, seed)
    res = engine.screen(model, dlib, topk=min(args.rows, len(dlib)))
    ex = engine.explain(model, dlib, res._best(min(args.rows, len(dlib))))
    rows, conf, keys = ex._own_rows(None)
    idx, conf, kb = engine._listed_rows(ex.indices[rows], conf, keys, "bench")
    n = len(idx)
    lib = _ffi.load()
    mh = engine.device_model(model, 0)
    w = engine._weights_array(None)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L, NN, NM, FW = 20, 64, 256, 4
    lig, cf, key = torch.from_numpy(idx).to(dev), torch.from_numpy(conf.astype(np.int32)).to(dev), torch.from_numpy(kb).to(dev)
    levels, status = torch.empty((n, L), dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    total = torch.empty(n, dtype=torch.float64, device=dev)
    node = torch.empty((n, NN), dtype=torch.float64, device=dev)
    entry, fails = torch.empty((n, L, L), dtype=torch.float32, device=dev), torch.empty((n, L, L), dtype=torch.int16, device=dev)
    share = torch.empty((n, NM), dtype=torch.float64, device=dev)
    terms, passes = torch.empty((n, NM), dtype=torch.int32, device=dev), torch.empty((n, NM), dtype=torch.int32, device=dev)
    fp = torch.empty((n, FW), dtype=torch.int64, device=dev)
    attribute = lambda: _ffi.check(lib.pmx_attribute(mh.handle, dlib.handle, w, lig.data_ptr(), cf.data_ptr(), key.data_ptr(), n, total.data_ptr(), node.data_ptr(),
                                                     entry.data_ptr(), fails.data_ptr(), levels.data_ptr(), status.data_ptr(), stream))
    hotspots = lambda: _ffi.check(lib.pmx_hotspots(mh.handle, dlib.handle, w, lig.data_ptr(), cf.data_ptr(), key.data_ptr(), n, total.data_ptr(), share.data_ptr(),
                                                   terms.data_ptr(), passes.data_ptr(), fp.data_ptr(), levels.data_ptr(), status.data_ptr(), stream))
    row = {"what": "tools/hotspots_bench.py: HIP-event ms of a warm call, best of 3", "ligands": len(dlib), "rows": n}
    row["attribute_ms"] = event_ms(torch, attribute)
    total_at = total.clone()
    row["hotspots_ms"] = event_ms(torch, hotspots)
    row["hotspots_over_attribute"] = row["hotspots_ms"] / row["attribute_ms"]
    row["totals_identical"] = bool(torch.equal(total_at.view(torch.int64), total.view(torch.int64)))
    row["rows_ok"] = int((status == 0).sum())
    row["mean_engaged_nodes"] = float(np.unpackbits(fp.cpu().numpy().view(np.uint8), axis=1).sum(axis=1).mean())
    row["mean_inner_terms"] = float(terms.sum(dim=1).double().mean()) / 2.0
    nb = min(args.against, n)
    sim = torch.empty((n, nb), dtype=torch.float32, device=dev)
    row["tanimoto_ms"] = event_ms(torch, lambda: _ffi.check(lib.pmx_fingerprint_tanimoto(fp.data_ptr(), n, fp.data_ptr(), nb, sim.data_ptr(), 0, stream)))
    row["tanimoto_block"] = [n, nb]
    row["tanimoto_GBps_written"] = n * nb * 4 / 1e9 / (row["tanimoto_ms"] / 1e3)
    del sim
    leader_of, leaders, count = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(2048, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    row["leaders_ms"] = event_ms(torch, lambda: _ffi.check(lib.pmx_fingerprint_leaders(fp.data_ptr(), n, args.threshold, 2048, leader_of.data_ptr(), leaders.data_ptr(),
                                                                                       count.data_ptr(), 0, stream)))
    row["leaders_threshold"] = args.threshold
    row["leaders_found"] = int(count.cpu()[0])
    row["leaders_unassigned"] = int((leader_of == -1).sum())
    row["csrc_sha16"] = bench.csrc_digest()
    row["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(row), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(row, indent=1) + "\n")


if __name__ == "__main__":
    main()
