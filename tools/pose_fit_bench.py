#!/usr/bin/env python3
"""What scoring a pose in place costs next to checking it: `pmx_pose_fit` in free mode and in key mode, and `pmx_pose_clash` in node mode -
the sibling call of the same launch shape - over the same rows of a resident synthetic library and the 6OIM pocket of tests/golden.

    python tools/pose_fit_bench.py [--ligands 4096] [--rows 65536] [--repeat 5]

`--ligands` ligands are generated, explained and fitted (`pmx_align`) once; the rows are those ligands at their best conformer under their
explaining key and the fit's own motion, repeated in order up to `--rows`. Device times between HIP events on the current stream, warm,
best and all of `--repeat` calls. Prints one JSON line."""
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
    new = lambda dt, *shape: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
    lig, cft, key = up(idx), up(cf.astype(np.int32)), up(kb)
    rot, trans, fit, node, cnt2, lv, st = new(f64, n, 9), new(f64, n, 3), new(f64, n, 8), new(f64, n, 64), new(i32, n, 2), new(torch.uint8, n, 20), new(i32, n)
    summary, count, ppen, patom, fp, cst = new(f64, n, 4), new(i32, n, 6), new(f64, n, 64), new(i32, n, 64), new(torch.int64, n, 4), new(i32, n)
    fsum, fcnt, nfit, nbest, nz2, ntgt = new(f64, n, 4), new(i32, n, 4), new(f64, n, 64), new(f64, n, 64), new(f64, n, 64), new(i32, n, 64)
    hz2, hnode, ofp, fst = new(f64, n, 256), new(i32, n, 256), new(torch.int64, n, 4), new(i32, n)
    mh, w = device_model(model, dlib.device), _weights_array(None)
    centers, sigmas = mh.node_centers(model), mh.node_sigmas(model)
    ph = device_pocket(pocket, dlib.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _ffi.check(lib.pmx_align(mh.handle, dlib.handle, w, centers.data_ptr(), lig.data_ptr(), cft.data_ptr(), key.data_ptr(), n, rot.data_ptr(), trans.data_ptr(), fit.data_ptr(),
                             node.data_ptr(), cnt2.data_ptr(), lv.data_ptr(), st.data_ptr(), stream))

    def clash():
        return lib.pmx_pose_clash(ph.handle, dlib.handle, lig.data_ptr(), cft.data_ptr(), None, None, None, rot.data_ptr(), trans.data_ptr(), n, 1.0, 0.5, 4.5, summary.data_ptr(),
                                  count.data_ptr(), ppen.data_ptr(), patom.data_ptr(), fp.data_ptr(), cst.data_ptr(), stream)

    def pose_fit(with_key):
        return lib.pmx_pose_fit(mh.handle, dlib.handle, w, centers.data_ptr(), sigmas.data_ptr(), lig.data_ptr(), cft.data_ptr(), key.data_ptr() if with_key else None, rot.data_ptr(),
                                trans.data_ptr(), n, fsum.data_ptr(), fcnt.data_ptr(), nfit.data_ptr(), nbest.data_ptr(), nz2.data_ptr(), ntgt.data_ptr(), hz2.data_ptr(), hnode.data_ptr(),
                                ofp.data_ptr(), fst.data_ptr(), stream)

    calls = {"pose_fit_free": lambda: pose_fit(False), "pose_fit_key": lambda: pose_fit(True), "clash_6oim": clash}
    out = dict(rows=n, ligands=len(dlib), mean_nodes=float(dlib._n_nodes[idx].mean()), model_nodes=int(model.num_nodes), pocket_atoms=len(pocket))
    for name, call in calls.items():
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
        if name.startswith("pose_fit"):
            ok = fst.cpu().numpy() == 0
            out[f"{name}_rows_ok"] = int(ok.sum())
            out[f"{name}_mean_pairs"] = float(fcnt.cpu().numpy()[ok, 1].mean()) if ok.any() else 0.0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
