#!/usr/bin/env python3
"""The record gather alone: `pmx_library_select` on the bench's resident libraries, against the two things it stands between.

    python tools/select_bench.py [--ligands 1000000] [--stress-ligands 100352] [--out profiles/r8_select.json]

Shapes: the identity list, a random permutation and a random 1 % subset of the 1 M-ligand synthetic library (8 conformers), and the identity
and a permutation of the 64-conformer stress library. Per shape, HIP-event times of a warm second call:

    select     the writing call as the C ABI offers it (sizes, scan, the host's one read, the record copy) into buffers that exist
    sizing     the sizing call alone (the same without the copy); copy = select - sizing is the copy kernel's share
    clone      (a) a torch device-to-device copy of the same number of bytes: the ceiling of a copy inside HBM
    host       (b) what there was before: NumPy gather of the host `PackedLibrary` + upload as a `DeviceLibrary` (wall clock)

profiles/r8_select.json also holds the A/B of the two copy mappings that decided for one wavefront per record.
GB/s count the selection's bytes once (a copy reads and writes them: the traffic is twice that)."""
import argparse
import ctypes
import json
import sys
import time
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


def measure(torch, engine, _ffi, dlib, host, idx, name):
    lib = _ffi.load()
    n = len(idx)
    idx_dev = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).cuda()
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    nbytes = ctypes.c_uint64(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _ffi.check(lib.pmx_library_select(dlib.handle, idx_dev.data_ptr(), n, offsets.data_ptr(), None, 0, ctypes.byref(nbytes), stream))
    total = int(nbytes.value)
    data = torch.empty(total, dtype=torch.uint8, device="cuda")
    sizing = lambda: _ffi.check(lib.pmx_library_select(dlib.handle, idx_dev.data_ptr(), n, offsets.data_ptr(), None, 0, ctypes.byref(nbytes), stream))
    writing = lambda: _ffi.check(lib.pmx_library_select(dlib.handle, idx_dev.data_ptr(), n, offsets.data_ptr(), data.data_ptr(), total, ctypes.byref(nbytes), stream))
    row = {"shape": name, "ligands": n, "bytes": total}
    row["sizing_ms"] = event_ms(torch, sizing)
    row["select_ms"] = event_ms(torch, writing)
    row["copy_ms"] = row["select_ms"] - row["sizing_ms"]
    src = dlib.buffers()[1][:total] if total <= dlib.num_bytes else None
    if src is not None:
        dst = torch.empty_like(src)
        row["clone_ms"] = event_ms(torch, lambda: dst.copy_(src))
        del dst
    if host is not None:
        t0 = time.perf_counter()
        up = engine.DeviceLibrary(host.select(idx))
        torch.cuda.synchronize()
        row["host_ms"] = (time.perf_counter() - t0) * 1e3
        same = bool(torch.equal(up.buffers()[1][:total], data)) and bool(torch.equal(up.buffers()[0], offsets))
        up.close()
        row["identical_to_host"] = same
    for k in ("select", "copy", "clone", "host"):
        if f"{k}_ms" in row:
            row[f"{k}_GBps"] = total / 1e9 / (row[f"{k}_ms"] / 1e3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ligands", type=int, default=1_000_000)
    ap.add_argument("--stress-ligands", type=int, default=100_352)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--no-host", action="store_true", help="leave out (b), the host gather and upload")
    args = ap.parse_args()
    import torch

    import bench
    from pharmaconet_amd import PackedLibrary, PharmacophoreModel, _ffi, engine

    rows = []
    rng = np.random.default_rng(20240811)
    for workload, n_lig in (("6oim", args.ligands), ("stress64", args.stress_ligands)):
        model_file, n_conf, _, topologies, active, seed = bench.WORKLOADS[workload]
        model = PharmacophoreModel.load(bench.REPO / "tests" / "golden" / model_file)
        dlib, offsets, data, _ = bench.build_library(model, n_lig, n_conf, topologies, 0, torch.device("cuda", 0), active, seed)
        host = PackedLibrary(offsets.cpu().numpy().view(np.uint64).copy(), data.cpu().numpy())
        del offsets, data
        n = len(dlib)
        shapes = {"identity": np.arange(n), "permutation": rng.permutation(n)}
        if workload == "6oim":
            shapes["subset_1pct"] = np.sort(rng.choice(n, n // 100, replace=False))
        for name, idx in shapes.items():
            row = measure(torch, engine, _ffi, dlib, None if args.no_host else host, idx, f"{workload}/{name}")
            print(json.dumps(row), flush=True)
            rows.append(row)
        dlib.close()
        del host
        torch.cuda.empty_cache()
    out = {"what": "tools/select_bench.py: pmx_library_select, HIP-event ms of a warm call; GB/s of the selection's bytes", "csrc_sha16": bench.csrc_digest(),
           "device": torch.cuda.get_device_name(0), "rows": rows}
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
