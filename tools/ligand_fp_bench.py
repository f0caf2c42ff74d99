#!/usr/bin/env python3
"""The ligand fingerprint pass and the similarity search alone, next to the floor they are compared with.

    python tools/ligand_fp_bench.py [--ligands 1000000] [--stress-ligands 100352] [--reps 7] [--out profiles/ligand_fp.json]

On the bench's resident libraries - the 1 M-ligand synthetic library (8 conformers) and the 64-conformer stress library - HIP-event times
of warm calls - per repeat a window of 10 calls (fingerprints, copy) or 100 (search), divided by that - every repeat kept (the spread is the
point of keeping them), the median quoted:

    fingerprints   `pmx_library_fingerprints` over the whole library: the union over the conformers, and one conformer per ligand
    copy           a device-to-device copy of the library's n_bytes (torch `copy_` of a contiguous uint8 buffer: one hipMemcpyAsync), taken
                   in the same run, alternating with the fingerprint call: the floor - the pass has to read every record once, the copy
                   reads and writes them
    search         `pmx_fingerprint_search` of nq = 1, 8 and 64 queries (library ligands, evenly spread) against the 1 M fingerprints

GB/s count the record bytes once (fingerprints, copy) or the bytes the search moves (32 n read, 4 n (nq + 1) written). Prints one JSON line.
`checksum` is the sum of the fingerprint words: two builds of the kernel that answer alike show the same one."""
import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))


def event_times(torch, fns, reps, inner):
    """HIP-event ms per call of each fn of `fns`: `reps` windows of `inner` calls each (a window of one short call would measure the events),
    the fns taken in turns (a, b, a, b, ...) after one warming call of each."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    seen = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(inner):
                fn()
            t1.record()
            torch.cuda.synchronize()
            seen[k].append(t0.elapsed_time(t1) / inner)
    return seen


def summary(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "ms_all": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ligands", type=int, default=1_000_000)
    ap.add_argument("--stress-ligands", type=int, default=100_352)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import torch

    import bench
    from pharmaconet_amd import PharmacophoreModel, _ffi, engine

    lib = _ffi.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {"what": "tools/ligand_fp_bench.py: HIP-event ms of warm calls, every repeat kept; GB/s of the record bytes (fingerprints, copy) or of the bytes moved (search)",
           "csrc_sha16": bench.csrc_digest(), "device": torch.cuda.get_device_name(0), "reps": args.reps, "calls_per_window": {"fingerprints": 10, "copy": 10, "search": 100}, "libraries": [], "search": []}
    for workload, n_lig in (("6oim", args.ligands), ("stress64", args.stress_ligands)):
        if n_lig <= 0:
            continue
        model_file, n_conf, _, topologies, active, seed = bench.WORKLOADS[workload]
        model = PharmacophoreModel.load(bench.REPO / "tests" / "golden" / model_file)
        dlib, offsets, data, _ = bench.build_library(model, n_lig, n_conf, topologies, 0, torch.device("cuda", 0), active, seed)
        del offsets
        n, nbytes = len(dlib), dlib.num_bytes
        bits = torch.empty((n, 4), dtype=torch.int64, device="cuda")
        counts = torch.empty((n, 8), dtype=torch.uint8, device="cuda")
        status = torch.empty(n, dtype=torch.int32, device="cuda")
        posed = torch.zeros(n, dtype=torch.int32, device="cuda")  # conformer 0 of every ligand
        src = data[:nbytes]
        dst = torch.empty_like(src)

        def fingerprints(conf=None):
            _ffi.check(lib.pmx_library_fingerprints(dlib.handle, 0, n, conf.data_ptr() if conf is not None else None, bits.data_ptr(), counts.data_ptr(), status.data_ptr(), stream))

        union_ms, copy_ms, posed_ms = event_times(torch, (fingerprints, lambda: dst.copy_(src), lambda: fingerprints(posed)), args.reps, 10)
        del dst
        fingerprints()
        torch.cuda.synchronize()
        row = {"library": workload, "ligands": n, "conformers": n_conf, "record_bytes": nbytes, "mean_nodes": float(counts[:, 7].float().mean()),
               "bits_per_ligand": float(sum(int(((bits >> s) & 1).sum()) for s in range(64)) / n), "unsupported": int((status != 0).sum()), "checksum": int(bits.sum()),
               "fingerprints": summary(union_ms), "copy": summary(copy_ms), "fingerprints_one_conformer": summary(posed_ms)}
        for k in ("fingerprints", "copy", "fingerprints_one_conformer"):
            row[k]["GBps"] = nbytes / 1e9 / (row[k]["ms_median"] / 1e3)
        row["fingerprints"]["ligands_per_s"] = n / (row["fingerprints"]["ms_median"] / 1e3)
        row["fingerprints_over_copy"] = row["fingerprints"]["ms_median"] / row["copy"]["ms_median"]
        print(json.dumps(row), flush=True)
        out["libraries"].append(row)
        if workload == "6oim":
            for nq in (1, 8, 64):
                query = bits[torch.linspace(0, n - 1, nq, device="cuda").long()].contiguous()
                sims = torch.empty((nq + 1, n), dtype=torch.float32, device="cuda")
                (ms,) = event_times(torch, (lambda: _ffi.check(lib.pmx_fingerprint_search(query.data_ptr(), nq, bits.data_ptr(), n, sims.data_ptr(), n, sims[nq].data_ptr(), 0, stream)),),
                                    args.reps, 100)
                moved = 32 * n + 4 * n * (nq + 1)
                srow = {"queries": nq, "fingerprints": n, **summary(ms), "bytes_moved": moved}
                srow["GBps"] = moved / 1e9 / (srow["ms_median"] / 1e3)
                srow["fingerprints_per_s"] = n / (srow["ms_median"] / 1e3)
                print(json.dumps(srow), flush=True)
                out["search"].append(srow)
                del sims
        dlib.close()
        del src, data, bits, counts, status, posed
        torch.cuda.empty_cache()
    engine.release_workspaces()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
