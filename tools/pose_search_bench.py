#!/usr/bin/env python3
"""What the pose search costs, and what composing it by hand costs: a pool of hits of the bench library (tools/synthetic.py, the generator
of tools/clash_bench.py) searched over every conformer under its M best binding modes against the 6OIM pocket of tests/golden.

    python tools/pose_search_bench.py [--hits 2048] [--modes 4] [--repeat 5]

`device_ms`: `pmx_explain_modes` + `pmx_pose_search` back to back on device tensors, between HIP events on the current stream, warm, best
and all of `--repeat` calls; `explain_modes_device_ms` and `pose_search_device_ms` are the two alone (the tree walk of the first depends on
the hits, not on the search). `composed_wall_ms`: the path without the call, in the same process - `engine.explain_modes`, `engine.align` and `engine.clashes` on the same slots (each goes device - NumPy - device), then the
rule in NumPy - as wall-clock time, warm, best and all of `--repeat`; its three stages are listed apart. `quotient` = composed_wall_ms /
wall_ms of `engine.pose_search`, the call a user makes (it includes the one download). The two paths' choices are compared before anything
is printed; `quotient_after_explain` leaves the tree walk, which both paths share, out: (composed - its explain_modes stage) /
pose_search_device_ms. Prints one JSON line."""
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


def composed(model, dlib, pocket, idx, modes, stride):
    """The search by hand: (conformer, mode) per hit and the wall-clock ms of the four stages."""
    from pharmaconet_amd.engine import align, clashes, explain_modes

    t = [time.perf_counter()]
    ms = explain_modes(model, dlib, idx, modes=modes)
    t.append(time.perf_counter())
    n = len(idx)
    v = np.zeros((n, modes, stride))
    for i in range(n):
        if ms.status[i] == 0:
            C = min(ms.values[i].shape[1], stride)
            v[i, :, :C] = ms.values[i][:, :C]
    live = v > 0
    conf = np.where(live, np.arange(stride)[None, None, :], -1).reshape(-1)
    lig = np.repeat(idx, modes * stride)
    empty = np.zeros(0, np.int64)
    keys = [ms.match[i][m, c] if live[i, m, c] else empty for i in range(n) for m in range(modes) for c in range(stride)]
    al = align(model, dlib, lig, conf, keys)
    t.append(time.perf_counter())
    rep = clashes(pocket, library=dlib, indices=lig, conformers=conf, rotation=al.rotation, translation=al.translation)
    t.append(time.perf_counter())
    cand = (live.reshape(-1) & (al.status == 0) & (al.n_nodes >= 1) & (rep.status == 0)).reshape(n, modes * stride)
    passing = cand & (rep.n_clashing <= 0).reshape(n, -1)
    c_of, m_of = np.tile(np.arange(stride), modes), np.repeat(np.arange(modes), stride)
    ov = np.where(passing, 0.0, rep.overlap.reshape(n, -1))
    choice = np.full((n, 2), -1)
    for i in range(n):
        s = np.flatnonzero(cand[i])
        if len(s):
            best = s[np.lexsort((m_of[s], c_of[s], -v[i].reshape(-1)[s], ov[i, s], ~passing[i, s]))[0]]
            choice[i] = c_of[best], m_of[best]
    t.append(time.perf_counter())
    return choice, [1e3 * (b - a) for a, b in zip(t, t[1:])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hits", type=int, default=2048)
    ap.add_argument("--modes", type=int, default=4)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    import torch

    from conftest import GOLDEN, load_golden
    from pharmaconet_amd import _ffi
    from pharmaconet_amd.engine import DeviceLibrary, _weights_array, device_model, device_pocket, pose_search
    from pharmaconet_amd.pocket import PocketAtoms
    from test_survey_library import _model_nodes
    from tools.synthetic import synthetic_library

    model, _, _, _ = load_golden("set_6oim_c8")
    dlib = DeviceLibrary(synthetic_library(a.hits, model_nodes=_model_nodes(model)))
    pocket = PocketAtoms.from_pdb(GOLDEN / "pocket_6oim.pdb", centers=model.node_centers)
    idx = np.arange(len(dlib), dtype=np.int64)
    n, M = len(idx), a.modes
    stride = int(np.clip(dlib._n_conf.max(), 1, 64))
    if n * M * stride > 65536:
        raise SystemExit(f"{n} hits x {M} modes x {stride} conformers is more than the 65536 slots of one call")

    lib = _ffi.load()
    dev = torch.device("cuda", dlib.device)
    f64, i32, u8 = torch.float64, torch.int32, torch.uint8
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)  # noqa: E731
    lig = torch.from_numpy(idx).to(dev)
    values, match, levels, best, est = new((n * M, 64), f64), new((n * M, 64, 20), u8), new((n, 20), u8), new(n, i32), new(n, i32)
    out = [new((n, 6), i32), new((n, 2), f64), new((n, 20), u8), new((n, 9), f64), new((n, 3), f64), new((n, 8), f64), new((n, 64), f64), new((n, 2), i32), new((n, 20), u8),
           new((n, 4), f64), new((n, 6), i32), new((n, 64), f64), new((n, 64), i32), new((n, 4), torch.int64), new(n, i32), new((2, n), i32)]
    need = int(lib.pmx_pose_search_work_bytes(n, M, stride))
    work = new(need, u8)
    mh, w = device_model(model, dlib.device), _weights_array(None)
    centers = mh.node_centers(model)
    ph = device_pocket(pocket, dlib.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def modes_call():
        return lib.pmx_explain_modes(mh.handle, dlib.handle, w, None, M, lig.data_ptr(), n, values.data_ptr(), match.data_ptr(), levels.data_ptr(), best.data_ptr(), est.data_ptr(),
                                     stream)

    def search_call():
        return lib.pmx_pose_search(mh.handle, dlib.handle, w, centers.data_ptr(), ph.handle, lig.data_ptr(), n, values.data_ptr(), match.data_ptr(), est.data_ptr(), M, stride, 1.0,
                                   0.5, 4.5, 0, 1, 0.0, *(t.data_ptr() for t in out), work.data_ptr(), need, stream)

    def both():
        return modes_call() or search_call()

    res = dict(hits=n, modes=M, conf_stride=stride, slots=n * M * stride, atoms=len(pocket), work_mb=round(need / 2**20, 1))
    for name, call in (("explain_modes_device_ms", modes_call), ("pose_search_device_ms", search_call), ("device_ms", both)):
        times = []
        for _ in range(a.repeat + 1):  # (the first is a warm-up)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _ffi.check(call())
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        res[name] = round(min(times[1:]), 3)
        res[name + "_all"] = [round(t, 3) for t in times[1:]]
    choice = out[0].cpu().numpy()
    res["posed"], res["passing"] = int((choice[:, 0] >= 0).sum()), int(choice[:, 2].sum())
    res["default_pose_chosen"] = int(((choice[:, 1] == 0) & (choice[:, 0] == best.cpu().numpy())).sum())

    walls, stages = [], []
    for _ in range(a.repeat + 1):
        t0 = time.perf_counter()
        ps = pose_search(model, dlib, pocket, idx, modes=M)
        walls.append(1e3 * (time.perf_counter() - t0))
    assert np.array_equal(ps.conformer, choice[:, 0]) and np.array_equal(ps.mode, choice[:, 1])
    for _ in range(a.repeat + 1):
        by_hand, st = composed(model, dlib, pocket, idx, M, stride)
        stages.append(st)
    assert np.array_equal(by_hand, choice[:, :2]), "the composed path chooses differently"
    res["wall_ms"], res["wall_ms_all"] = round(min(walls[1:]), 2), [round(t, 2) for t in walls[1:]]
    totals = [sum(s) for s in stages[1:]]
    res["composed_wall_ms"], res["composed_wall_ms_all"] = round(min(totals), 2), [round(t, 2) for t in totals]
    res["composed_stages_ms"] = dict(zip(("explain_modes", "align", "clashes", "rule"), (round(v, 2) for v in stages[1 + int(np.argmin(totals))])))
    res["quotient"] = round(res["composed_wall_ms"] / res["wall_ms"], 2)
    res["quotient_after_explain"] = round((res["composed_wall_ms"] - res["composed_stages_ms"]["explain_modes"]) / res["pose_search_device_ms"], 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
