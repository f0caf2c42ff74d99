#!/usr/bin/env python3
"""Retrospective validation alone: `pmx_enrichment` on the bench library's scores, against the only route there was before it.

    python tools/enrichment_bench.py [--ligands 1000000] [--bootstrap 1000] [--out profiles/enrichment.json]

The 1 M-ligand synthetic library of bench.py (8 conformers) is scored under four weight sets (`engine.sweep`'s buffer: [4, n] float32 on the
device); one ligand in a hundred, drawn at random, is called an active - the timings depend on the tie structure of real scores, not on
which ligands carry the label. Per bootstrap count (0 and --bootstrap), of a warm call, the best of --reps (all of them are kept):

    enrichment_ms   HIP-event time of pmx_enrichment, and its split as the call's own events give it (pmx_set_profiling(1),
                    pmx_enrichment_times): totals | keys + sort | ranked-byte pass | walk
    host_ms         the route without it, by wall clock: download of the four columns, NumPy argsort per column and row 0 of the
                    restatement (tests/enrichment_ref.py) - no bootstrap at all

Prints one JSON line."""
import argparse
import ctypes
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

WEIGHT_SETS = (
    None,
    dict(Hydrophobic=2.0),
    dict(Aromatic=2.0, HBond_donor=6.0, HBond_acceptor=6.0),
    dict(Cation=4.0, Anion=4.0, Halogen=1.0),
)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ligands", type=int, default=1_000_000)
    ap.add_argument("--bootstrap", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--no-host", action="store_true", help="leave out the host route")
    args = ap.parse_args()
    import torch

    import bench
    import enrichment_ref as ref
    from pharmaconet_amd import PharmacophoreModel, _ffi, engine

    model_file, n_conf, _, topologies, active, seed = bench.WORKLOADS["6oim"]
    model = PharmacophoreModel.load(REPO / "tests" / "golden" / model_file)
    dlib, offsets, data, _ = bench.build_library(model, args.ligands, n_conf, topologies, 0, torch.device("cuda", 0), active, seed)
    n = len(dlib)
    labels = (np.random.default_rng(20241019).random(n) < 0.01).astype(np.uint8)
    cutoffs = (0.005, 0.01, 0.05)
    en0, scores = engine.sweep([model], dlib, labels, WEIGHT_SETS, cutoffs=cutoffs, return_scores=True)
    lib = _ffi.load()
    lab = torch.from_numpy(labels).cuda()
    ppm = engine.cutoffs_ppm(cutoffs)
    cut = (ctypes.c_uint32 * len(ppm))(*(int(p) for p in ppm))
    n_cols = int(scores.shape[0])
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {"what": "tools/enrichment_bench.py: pmx_enrichment, HIP-event ms of a warm call (best of reps) and its phases; host_ms: download + argsort + row 0 in NumPy, wall clock",
           "csrc_sha16": bench.csrc_digest(), "device": torch.cuda.get_device_name(0), "ligands": n, "columns": n_cols, "n_active": int(labels.sum()),
           "tie_groups": [int(len(np.unique(scores[c].cpu().numpy()))) for c in range(n_cols)], "auroc": [float(v) for v in en0.auroc], "rows": []}
    engine.set_profiling(True)
    for boot in (0, args.bootstrap):
        rows = 1 + boot
        totals = torch.empty((rows, 3), dtype=torch.int64, device="cuda")
        u2 = torch.empty((n_cols, rows), dtype=torch.int64, device="cuda")
        hits = torch.empty((n_cols, rows, len(ppm)), dtype=torch.float64, device="cuda")
        expsum = torch.empty((n_cols, rows), dtype=torch.float64, device="cuda")

        def call():
            _ffi.check(lib.pmx_enrichment(scores.data_ptr(), int(scores.stride(0)), n_cols, n, None, lab.data_ptr(), cut, len(ppm), 20.0, boot, 1, totals.data_ptr(),
                                          u2.data_ptr(), hits.data_ptr(), expsum.data_ptr(), None, 0, 0, stream))

        call()  # warm: the work buffers exist afterwards
        torch.cuda.synchronize()
        best, phases, seen = 1e30, None, []
        for _ in range(args.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            call()
            t1.record()
            torch.cuda.synchronize()
            ms = (ctypes.c_double * 4)()
            _ffi.check(lib.pmx_enrichment_times(0, ms))
            seen.append(t0.elapsed_time(t1))
            if t0.elapsed_time(t1) < best:
                best, phases = t0.elapsed_time(t1), list(ms)
        out["rows"].append({"bootstrap": boot, "enrichment_ms": best, "enrichment_ms_all": seen, "totals_ms": phases[0], "sort_ms": phases[1], "ranked_ms": phases[2], "walk_ms": phases[3],
                            "walk_positions_per_s": n * n_cols * rows / (phases[3] / 1e3)})
    engine.set_profiling(False)
    if not args.no_host:
        best = 1e30
        for _ in range(min(args.reps, 2)):
            t0 = time.perf_counter()
            host = scores.cpu().numpy()
            got = ref.enrichment_ref(host, labels, None, ppm, 20.0, 0, 0)
            best = min(best, (time.perf_counter() - t0) * 1e3)
        out["host_ms"] = best
        out["host_equals_device_row0"] = bool((got["u2"][:, 0] == en0.u2[:, 0]).all() and (got["hits"][:, 0].view(np.uint64) == en0.hits[:, 0].view(np.uint64)).all())
    print(json.dumps(out), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
