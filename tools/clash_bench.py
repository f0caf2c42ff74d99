#!/usr/bin/env python3
"""What a pose check costs next to the fit it follows: `pmx_pose_clash` in node mode over 65536 rows of the bench library's generator,
against the 6OIM pocket of tests/golden and against a pocket of 5000 atoms, and `pmx_align` of the same rows.

    python tools/clash_bench.py [--ligands 4096] [--rows 65536] [--repeat 5]

`--ligands` ligands are generated and explained once; the rows are those ligands at their best conformer under their explaining key,
repeated in order up to `--rows`. Device times between HIP events on the current stream, warm, best and all of `--repeat` calls.
(csrc/pmx_rows.hip decides `pmx_align`'s time; a build whose pmx_rows.hip is the parent commit's measures the parent's.) Prints one JSON line."""
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

    pockets = {"6oim": PocketAtoms.from_pdb(GOLDEN / "pocket_6oim.pdb", centers=model.node_centers)}
    rng = np.random.default_rng(0)
    centre = model.node_centers.mean(axis=0)
    ball = rng.normal(size=(5000, 3))
    ball *= (30.0 * rng.random(5000) ** (1 / 3) / np.linalg.norm(ball, axis=1))[:, None]  # uniform in a ball of 30 A: 0.044 atoms / A^3, a protein's density
    pockets["5000"] = PocketAtoms.from_arrays(ball + centre, np.full(5000, 1.7), rng.integers(0, 256, 5000))

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
    mh, w = device_model(model, dlib.device), _weights_array(None)
    centers = mh.node_centers(model)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def align():
        return lib.pmx_align(mh.handle, dlib.handle, w, centers.data_ptr(), lig.data_ptr(), cft.data_ptr(), key.data_ptr(), n, rot.data_ptr(), trans.data_ptr(), fit.data_ptr(),
                             node.data_ptr(), cnt2.data_ptr(), lv.data_ptr(), st.data_ptr(), stream)

    def clash(ph, with_fp=True):
        return lib.pmx_pose_clash(ph.handle, dlib.handle, lig.data_ptr(), cft.data_ptr(), None, None, None, rot.data_ptr(), trans.data_ptr(), n, 1.0, 0.5, 4.5, summary.data_ptr(),
                                  count.data_ptr(), ppen.data_ptr(), patom.data_ptr(), fp.data_ptr() if with_fp else None, cst.data_ptr(), stream)

    calls = {"align": align}
    for name, pocket in pockets.items():
        ph = device_pocket(pocket, dlib.device)
        calls[f"clash_{name}"] = lambda ph=ph: clash(ph)
        calls[f"clash_{name}_no_fingerprint"] = lambda ph=ph: clash(ph, False)
    out = dict(rows=n, ligands=len(dlib), mean_nodes=float(dlib._n_nodes[idx].mean()),
               atoms={k: len(p) for k, p in pockets.items()})
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
        if name.startswith("clash") and not name.endswith("fingerprint"):
            ok = cst.cpu().numpy() == 0
            out[f"{name}_rows_ok"] = int(ok.sum())
            out[f"{name}_rows_clashing"] = int((count.cpu().numpy()[ok, 1] > 0).sum())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
