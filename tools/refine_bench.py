#!/usr/bin/env python3
"""What a refinement costs next to the check it contains: `pmx_pose_refine` in node mode over the 65536 rows of tools/clash_bench.py - the
bench library's generator, each ligand at its best conformer under its explaining key, fitted by `pmx_align` - against the 6OIM pocket of
tests/golden, and `pmx_pose_clash` on the same rows in the same run.

    python tools/refine_bench.py [--ligands 4096] [--rows 65536] [--repeat 5] [--max_iter 32] [--restraint 0.1]

Device times between HIP events on the current stream, warm, best and all of `--repeat` calls. `mean_evaluations` is the mean of the
rows' `iterations`: an upper bound, since a trial whose Cholesky pivot is not positive counts as an iteration without an evaluation
(`rejected_without_evaluation_bound` says how many rows could have had one: those that stopped for want of a step). `quotient` is refine
time / ((mean evaluations + 1) x clash time): what an evaluation costs relative to the check it contains (an evaluation of a row is a walk over the
pocket's atoms like the check's, with the normal equations on top; the + 1 is the evaluation at the start). `failing_to_passing` is the
share of the rows failing `ClashReport.ok()` before that pass it after, at the same tolerance and at a refinement tolerance of 0.
Prints one JSON line."""
import argparse
import ctypes
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ligands", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--max_iter", type=int, default=32)
    ap.add_argument("--restraint", type=float, default=0.1)
    a = ap.parse_args()
    import torch

    from conftest import GOLDEN, load_golden
    from pharmaconet_amd import _ffi
    from pharmaconet_amd.engine import DeviceLibrary, _listed_rows, _weights_array, device_model, device_pocket, explain
    from pharmaconet_amd.pocket import PocketAtoms
    from test_survey_library import _model_nodes
    from tools.synthetic import synthetic_library

    model, _, _, _ = load_golden("set_6oim_c8")
    dlib = DeviceLibrary(synthetic_library(a.ligands, model_nodes=_model_nodes(model)))
    ex = explain(model, dlib, np.arange(len(dlib)))
    own, conf, keys = ex._own_rows(None)
    take = np.resize(np.arange(len(own)), a.rows)
    idx, cf, kb = _listed_rows(ex.indices[own][take], np.asarray(conf)[take], [keys[j] for j in take], "align")
    n = len(idx)
    pocket = PocketAtoms.from_pdb(GOLDEN / "pocket_6oim.pdb", centers=model.node_centers)

    lib = _ffi.load()
    dev = torch.device("cuda", dlib.device)
    f64, i32 = torch.float64, torch.int32
    up = lambda x: torch.from_numpy(x).to(dev)  # noqa: E731
    lig, cft, key = up(idx), up(cf.astype(np.int32)), up(kb)
    rot, trans, fit = torch.empty((n, 9), dtype=f64, device=dev), torch.empty((n, 3), dtype=f64, device=dev), torch.empty((n, 8), dtype=f64, device=dev)
    node, cnt2 = torch.empty((n, 64), dtype=f64, device=dev), torch.empty((n, 2), dtype=i32, device=dev)
    lv, st = torch.empty((n, 20), dtype=torch.uint8, device=dev), torch.empty(n, dtype=i32, device=dev)
    summary, count = torch.empty((n, 4), dtype=f64, device=dev), torch.empty((n, 6), dtype=i32, device=dev)
    ppen, patom = torch.empty((n, 64), dtype=f64, device=dev), torch.empty((n, 64), dtype=i32, device=dev)
    fp, cst = torch.empty((n, 4), dtype=torch.int64, device=dev), torch.empty(n, dtype=i32, device=dev)
    rot2, trans2, energy = torch.empty((n, 9), dtype=f64, device=dev), torch.empty((n, 3), dtype=f64, device=dev), torch.empty((n, 8), dtype=f64, device=dev)
    rcount, rst = torch.empty((n, 4), dtype=i32, device=dev), torch.empty(n, dtype=i32, device=dev)
    mh, w = device_model(model, dlib.device), _weights_array(None)
    centers = mh.node_centers(model)
    ph = device_pocket(pocket, dlib.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _ffi.check(lib.pmx_align(mh.handle, dlib.handle, w, centers.data_ptr(), lig.data_ptr(), cft.data_ptr(), key.data_ptr(), n, rot.data_ptr(), trans.data_ptr(), fit.data_ptr(),
                             node.data_ptr(), cnt2.data_ptr(), lv.data_ptr(), st.data_ptr(), stream))

    def clash(r=rot, t=trans):
        return lib.pmx_pose_clash(ph.handle, dlib.handle, lig.data_ptr(), cft.data_ptr(), None, None, None, r.data_ptr(), t.data_ptr(), n, 1.0, 0.5, 4.5, summary.data_ptr(),
                                  count.data_ptr(), ppen.data_ptr(), patom.data_ptr(), fp.data_ptr(), cst.data_ptr(), stream)

    def refine(tolerance=0.5, max_iter=a.max_iter):
        return lib.pmx_pose_refine(ph.handle, dlib.handle, lig.data_ptr(), cft.data_ptr(), None, None, None, None, None, None, None, rot.data_ptr(), trans.data_ptr(), n, 1.0,
                                   tolerance, a.restraint, 1e-9, max_iter, rot2.data_ptr(), trans2.data_ptr(), energy.data_ptr(), rcount.data_ptr(), rst.data_ptr(), stream)

    out = dict(rows=n, ligands=len(dlib), mean_nodes=float(dlib._n_nodes[idx].mean()), atoms=len(pocket), max_iter=a.max_iter, restraint=a.restraint)
    for name, call in (("clash", clash), ("refine", refine), ("refine_iter0", lambda: refine(max_iter=0))):
        times = []
        for _ in range(a.repeat + 1):  # (the first is a warm-up)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _ffi.check(call())
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        out[f"{name}_device_ms"] = round(min(times[1:]), 3)
        out[f"{name}_device_ms_all"] = [round(t, 3) for t in times[1:]]
    _ffi.check(clash())
    torch.cuda.synchronize(dev)
    ok = cst.cpu().numpy() == 0
    failing = ok & (count.cpu().numpy()[:, 1] > 0)
    out["rows_ok"], out["rows_failing_before"] = int(ok.sum()), int(failing.sum())
    for tag, tol in (("", 0.5), ("_at_tolerance_0", 0.0)):
        _ffi.check(refine(tolerance=tol))
        _ffi.check(clash(rot2, trans2))
        torch.cuda.synchronize(dev)
        rc, en = rcount.cpu().numpy(), energy.cpu().numpy()
        passing = failing & (count.cpu().numpy()[:, 1] == 0) & (cst.cpu().numpy() == 0)
        if not tag:
            evals = rc[ok, 0].astype(np.float64)
            out["mean_evaluations"] = float(evals.mean())
            out["mean_evaluations_of_clashing_rows"] = float(rc[failing, 0].mean()) if failing.any() else 0.0
            out["rejected_without_evaluation_bound"] = int((rc[ok, 2] == 3).sum())
            out["stops"] = {str(k): int((rc[ok, 2] == k).sum()) for k in range(4)}
            out["quotient"] = out["refine_device_ms"] / ((out["mean_evaluations"] + 1.0) * out["clash_device_ms"])
        out[f"failing_to_passing{tag}"] = float(passing.sum() / max(int(failing.sum()), 1))
        out[f"anchor_rmsd_of_those{tag}"] = [float(v) for v in np.percentile(en[passing, 4], [50, 90, 100])] if passing.any() else []
        out[f"anchor_rmsd_of_failing{tag}"] = [float(v) for v in np.percentile(en[failing, 4], [50, 90, 100])] if failing.any() else []
        out[f"overlap_of_failing_before_after{tag}"] = [float(np.median(en[failing, 0])), float(np.median(en[failing, 2]))] if failing.any() else []
    print(json.dumps(out))


if __name__ == "__main__":
    main()
