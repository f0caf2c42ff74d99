#!/usr/bin/env python3
"""Time of `engine.explain` for the top hits of a screen (the cost of inspecting them, include/pmx.h pmx_explain).

    python tools/explain_bench.py [--ligands 1000000] [--hits 1000] [--library bench|survey|stress] [--repeat 3]

Scores the library once (pmx_score_f64), ranks it on the host and times explain of the `--hits` best ligands on a resident library,
best of `--repeat` calls after one warm-up call. Prints one JSON line."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ligands", type=int, default=1_000_000)
    ap.add_argument("--hits", type=int, default=1000)
    ap.add_argument("--library", choices=("bench", "survey", "stress"), default="bench")
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    import torch

    from conftest import load_golden
    from pharmaconet_amd import PackedLibrary
    from pharmaconet_amd.engine import DeviceLibrary, explain, last_score_stats, screen

    import bench

    if a.library == "stress":
        model, lib, weights, _ = load_golden("set_s64_c64")
        lib = PackedLibrary.from_records([lib.record(i % len(lib)) for i in range(a.ligands)])
        dlib = DeviceLibrary(lib)
    else:
        model, _, _, _ = load_golden("set_6oim_c8")
        weights = None
        if a.library == "survey":
            _, off, data, _ = bench.build_survey_library(model, a.ligands, 8, 0, "cuda:0")
        else:
            _, off, data, _ = bench.build_library(model, a.ligands, 8, min(a.ligands, 4096), 0, "cuda:0")
        dlib = DeviceLibrary.from_device_buffers(off, data, "cuda:0", adopt=True)  # (explain reads conformer counts from the records)
    res = screen(model, dlib, weights=weights, float64=True)
    stats = last_score_stats()  # (the score pass's longest single walk and its split trees, for comparison with the explain time)
    sc = res.scores.cpu().numpy()
    key = np.where(res.status.cpu().numpy() != 0, -np.inf, sc)
    top = np.lexsort((np.arange(len(sc)), -key))[: a.hits]
    ex = explain(model, dlib, top, weights=weights)  # warm-up (workspace, tables of the pair functions)
    times = []
    for _ in range(a.repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ex = explain(model, dlib, top, weights=weights)
        times.append(time.perf_counter() - t0)
    means = np.array([m.mean() for m in ex.conf_max])
    print(json.dumps(dict(library=a.library, ligands=dlib.num_ligands, hits=len(top), explain_ms=round(1e3 * min(times), 3),
                          explain_ms_all=[round(1e3 * t, 3) for t in times], max_abs_diff_vs_score=float(np.abs(means - sc[top]).max()),
                          misses=int((ex.status == 3).sum()),
                          score_pass_longest_walk=int(stats["max_passes"]), score_pass_split_trees=int(stats["n_heavy"]))))


if __name__ == "__main__":
    main()
