#!/usr/bin/env python3
"""What constrained matching costs, on the 4096-ligand slice of the bench library's generator that the explain tests use.

    python tools/constrained_bench.py [--ligands 4096] [--repeat 5] [--topk 100]

Device times between HIP events on the current stream, warm, best and spread of `--repeat` calls: `pmx_explain` of every ligand,
`pmx_explain_constrained` with one require group (the cluster most often matched in the unconstrained keys) and with an exclude set
(the same cluster), and the wall time of `engine.screen_constrained` for `--topk` hits next to a plain `engine.screen`. With
`PMX_LIBPMX` pointing at a build without `pmx_explain_constrained` (an A/B against an older library) only `pmx_explain` is timed.
Prints one JSON line."""
import argparse
import ctypes
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
    ap.add_argument("--ligands", type=int, default=4096)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--topk", type=int, default=100)
    a = ap.parse_args()
    import os

    import torch

    from pharmaconet_amd import _ffi

    has = True
    if os.environ.get("PMX_LIBPMX"):
        torch.zeros(1)  # (torch's HIP runtime first, as _ffi.load does)
        has = hasattr(ctypes.CDLL(os.environ["PMX_LIBPMX"]), "pmx_explain_constrained")
        if not has:
            _ffi.SIGNATURES.pop("pmx_explain_constrained")
    from conftest import load_golden
    from pharmaconet_amd.engine import DeviceLibrary, _constraint_struct, _weights_array, device_model, explain, screen, screen_constrained
    from test_survey_library import _model_nodes
    from tools.synthetic import synthetic_library

    model, _, _, _ = load_golden("set_6oim_c8")
    dlib = DeviceLibrary(synthetic_library(a.ligands, model_nodes=_model_nodes(model)))
    n = len(dlib)
    base = explain(model, dlib, np.arange(n))
    count = np.zeros(model.flat.num_clusters, np.int64)
    for r in range(n):
        if base.status[r] == 0:
            m = base.match[r]
            count[np.unique(m[m >= 0])] += 1
    common = int(np.argmax(count))

    lib = _ffi.load()
    dev = torch.device("cuda", dlib.device)
    f64, u8, i32 = torch.float64, torch.uint8, torch.int32
    lig = torch.arange(n, dtype=torch.int64, device=dev)
    cm, mt, lv = torch.empty((n, 64), dtype=f64, device=dev), torch.empty((n, 64, 20), dtype=u8, device=dev), torch.empty((n, 20), dtype=u8, device=dev)
    best, st = torch.empty(n, dtype=i32, device=dev), torch.empty(n, dtype=i32, device=dev)
    mh, w = device_model(model, dlib.device), _weights_array(None)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    outs = (lig.data_ptr(), n, cm.data_ptr(), mt.data_ptr(), lv.data_ptr(), best.data_ptr(), st.data_ptr(), stream)
    calls = {"explain": lambda: lib.pmx_explain(mh.handle, dlib.handle, w, *outs)}
    if has:
        for name, con in (("require", _constraint_struct(((common,),), ())), ("exclude", _constraint_struct((), (common,)))):
            calls[name] = lambda con=con: lib.pmx_explain_constrained(mh.handle, dlib.handle, w, ctypes.byref(con), *outs)
    out = dict(ligands=n, cluster=common, ligands_matching_it=int(count[common]), constrained_symbol=has)
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
        if name != "explain":
            out[f"{name}_positive_rows"] = int((cm[:, :8].sum(dim=1) > 0).sum())
    if has:
        def wall(f):
            f()
            times = []
            for _ in range(a.repeat):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = f()
                torch.cuda.synchronize()
                times.append(1e3 * (time.perf_counter() - t0))
            return r, times

        _, t_plain = wall(lambda: screen(model, dlib, topk=a.topk))
        for name, kw in (("require", dict(require=[[common]])), ("exclude", dict(exclude=[common]))):
            r, t = wall(lambda kw=kw: screen_constrained(model, dlib, a.topk, **kw))
            out[f"screen_constrained_{name}_ms"] = round(min(t), 3)
            out[f"screen_constrained_{name}_ms_all"] = [round(x, 3) for x in t]
            out[f"screen_constrained_{name}_pool"] = r.pool
            out[f"screen_constrained_{name}_exact"] = r.exact
        out["screen_ms"] = round(min(t_plain), 3)
        out["screen_ms_all"] = [round(x, 3) for x in t_plain]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
