#!/usr/bin/env python3
"""Time of `engine.explain` for the top hits of a screen (the cost of inspecting them, include/pmx.h pmx_explain).

    python tools/explain_bench.py [--ligands 1000000] [--hits 1000] [--library bench|survey|stress] [--repeat 3] [--attribute] [--align]

Scores the library once (pmx_score_f64), ranks it on the host and times explain of the `--hits` best ligands on a resident library,
best of `--repeat` calls after one warm-up call. With `--attribute` also `engine.attribute` of the same hits at their best conformer under
their own key (`Explanation.attribution`), and - the host's packing and cutting of 65 536 rows being most of either wall time - the device
time of the two C calls alone between HIP events. With `--align` the same for `engine.align` (`Explanation.poses`, pmx_align). Prints one JSON line."""
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
    ap.add_argument("--attribute", action="store_true", help="also time engine.attribute of the same hits")
    ap.add_argument("--align", action="store_true", help="also time engine.align of the same hits")
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
    extra = {}
    if a.attribute:
        at = ex.attribution(model, dlib, weights=weights)  # warm-up
        wall = []
        for _ in range(a.repeat):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            at = ex.attribution(model, dlib, weights=weights)
            wall.append(time.perf_counter() - t0)
        extra = dict(attribute_rows=len(at), attribute_ms=round(1e3 * min(wall), 3), attribute_invalid=int((at.status != 0).sum()), **device_times(model, dlib, weights, ex, a.repeat))
    if a.align:
        al = ex.poses(model, dlib, weights=weights)  # warm-up (the node centres go to the device)
        wall = []
        for _ in range(a.repeat):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            al = ex.poses(model, dlib, weights=weights)
            wall.append(time.perf_counter() - t0)
        extra.update(align_rows=len(al), align_ms=round(1e3 * min(wall), 3), align_invalid=int((al.status != 0).sum()),
                     **device_times(model, dlib, weights, ex, a.repeat, ("explain_device_ms", "align_device_ms")))
    means = np.array([m.mean() for m in ex.conf_max])
    print(json.dumps(dict(**extra, library=a.library, ligands=dlib.num_ligands, hits=len(top), explain_ms=round(1e3 * min(times), 3),
                          explain_ms_all=[round(1e3 * t, 3) for t in times], max_abs_diff_vs_score=float(np.abs(means - sc[top]).max()),
                          misses=int((ex.status == 3).sum()),
                          score_pass_longest_walk=int(stats["max_passes"]), score_pass_split_trees=int(stats["n_heavy"]))))


def device_times(model, dlib, weights, ex, repeat, which=("explain_device_ms", "attribute_device_ms")):
    """pmx_explain, pmx_attribute and pmx_align (those of `which`) of the explanation's OK rows between HIP events on the current stream:
    best of `repeat`, in ms."""
    import ctypes

    import torch

    from pharmaconet_amd import _ffi
    from pharmaconet_amd.engine import _weights_array, device_model

    lib = _ffi.load()
    dev = torch.device("cuda", dlib.device)
    rows = [i for i in range(len(ex)) if ex.status[i] == 0]
    n = len(rows)
    keys = np.full((n, 20), 0xFF, np.uint8)
    for r, i in enumerate(rows):
        k = ex.match[i][int(ex.best_conformer[i])]
        keys[r, : len(k)] = np.where(k < 0, 0xFF, k)
    lig = torch.from_numpy(ex.indices[rows].astype(np.int64)).to(dev)
    conf = torch.from_numpy(ex.best_conformer[rows].astype(np.int32)).to(dev)
    key = torch.from_numpy(keys).to(dev)
    f64, u8, i32 = torch.float64, torch.uint8, torch.int32
    cm, mt, lv = torch.empty((n, 64), dtype=f64, device=dev), torch.empty((n, 64, 20), dtype=u8, device=dev), torch.empty((n, 20), dtype=u8, device=dev)
    best, st = torch.empty(n, dtype=i32, device=dev), torch.empty(n, dtype=i32, device=dev)
    tot, nd = torch.empty(n, dtype=f64, device=dev), torch.empty((n, 64), dtype=f64, device=dev)
    en, fl = torch.empty((n, 20, 20), dtype=torch.float32, device=dev), torch.empty((n, 20, 20), dtype=torch.int16, device=dev)
    rot, tr, fit = torch.empty((n, 9), dtype=f64, device=dev), torch.empty((n, 3), dtype=f64, device=dev), torch.empty((n, 8), dtype=f64, device=dev)
    cnt = torch.empty((n, 2), dtype=i32, device=dev)
    mh, w = device_model(model, dlib.device), _weights_array(weights)
    ctr = mh.node_centers(model)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    calls = dict(
        explain_device_ms=lambda: lib.pmx_explain(mh.handle, dlib.handle, w, lig.data_ptr(), n, cm.data_ptr(), mt.data_ptr(), lv.data_ptr(), best.data_ptr(), st.data_ptr(), stream),
        attribute_device_ms=lambda: lib.pmx_attribute(mh.handle, dlib.handle, w, lig.data_ptr(), conf.data_ptr(), key.data_ptr(), n, tot.data_ptr(), nd.data_ptr(),
                                                      en.data_ptr(), fl.data_ptr(), lv.data_ptr(), st.data_ptr(), stream),
        align_device_ms=lambda: lib.pmx_align(mh.handle, dlib.handle, w, ctr.data_ptr(), lig.data_ptr(), conf.data_ptr(), key.data_ptr(), n, rot.data_ptr(), tr.data_ptr(),
                                              fit.data_ptr(), nd.data_ptr(), cnt.data_ptr(), lv.data_ptr(), st.data_ptr(), stream),
    )
    out = {}
    for name, call in calls.items():
        if name not in which:
            continue
        times = []
        for _ in range(repeat + 1):  # (the first is a warm-up)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _ffi.check(call())
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        out[name] = round(min(times[1:]), 3)
        out[name + "_all"] = [round(t, 3) for t in times[1:]]
    return out


if __name__ == "__main__":
    main()
