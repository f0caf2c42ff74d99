#!/usr/bin/env python3
"""What the atom store costs and saves, on the bench generator's molecules against the 6OIM pocket of tests/golden:

  (a) `pmx_atoms_gather` alone, `--rows` rows: device time
  (b) `clashes(atoms=store)` against the list-of-molecules path (`_heavy_atoms` on the host, then `clashes(points=...)`) on the same rows and
      motions: wall clock around the whole call, the two alternating
  (c) `pmx_pose_search_atoms` against `pmx_pose_search` on the same `--rows` slots (hits x 4 modes x 8 conformers): device time

    python tools/atoms_bench.py [--ligands 1024] [--rows 65536] [--repeat 5]

One process, warm (one call of each before the timed ones), best and all of `--repeat`. Prints one JSON line."""
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
    ap.add_argument("--ligands", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    import torch

    from conftest import GOLDEN, load_golden
    from pharmaconet_amd import _ffi
    from pharmaconet_amd.atoms import PackedAtoms
    from pharmaconet_amd.engine import (DeviceAtoms, DeviceLibrary, _explain_call, _heavy_atoms, _weights_array, clashes, device_model, device_pocket, explain)
    from pharmaconet_amd.pocket import PocketAtoms
    from test_survey_library import _model_nodes
    from tools.synthetic import synthetic_library

    model, _, _, _ = load_golden("set_6oim_c8")
    mols = []
    packed = synthetic_library(a.ligands, model_nodes=_model_nodes(model), molecules_out=mols)
    store = PackedAtoms.for_library(mols, packed)
    dlib, dat = DeviceLibrary(packed), DeviceAtoms(store)
    pocket = PocketAtoms.from_pdb(GOLDEN / "pocket_6oim.pdb", centers=model.node_centers)
    al = explain(model, dlib, np.arange(len(dlib))).poses(model, dlib)
    ok = np.flatnonzero(al.status == 0)
    take = ok[np.resize(np.arange(len(ok)), a.rows)]
    idx, conf, rot, trans = al.indices[take].astype(np.int64), np.asarray(al.conformers)[take].astype(np.int64), al.rotation[take], al.translation[take]
    n = len(idx)
    out = dict(rows=n, ligands=len(dlib), pocket_atoms=len(pocket), store_bytes=dat.num_bytes, max_atoms=dat.max_atoms,
               points_per_row=float(store.headers()[idx, 0].mean()))

    dev = torch.device("cuda", dlib.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def device_ms(call):
        times = []
        for _ in range(a.repeat + 1):  # (the first is a warm-up)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        return round(min(times[1:]), 3), [round(t, 3) for t in times[1:]]

    # (a) the gather alone
    lig, cf = torch.from_numpy(idx).to(dev), torch.from_numpy(conf.astype(np.int32)).to(dev)
    out["gather_device_ms"], out["gather_device_ms_all"] = device_ms(lambda: dat.gather_device(lig, cf, n))

    # (b) the check from the store against the check from a list of molecules, wall clock, alternating
    listed = [mols[int(i)] for i in idx]

    def from_store():
        return clashes(pocket, atoms=dat, indices=idx, conformers=conf, rotation=rot, translation=trans)

    def from_list():
        points, radii = _heavy_atoms(listed, conf)
        return clashes(pocket, points=points, point_radii=radii, rotation=rot, translation=trans)

    same = np.array_equal(from_store().overlap, from_list().overlap, equal_nan=True)  # (warm-up, and the two ways agree)
    wall = {"store": [], "list": []}
    for _ in range(a.repeat):
        for name, call in (("store", from_store), ("list", from_list)):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            call()
            wall[name].append((time.perf_counter() - t0) * 1e3)
    out.update(clashes_same_bits=bool(same), clashes_store_wall_ms=round(min(wall["store"]), 2), clashes_store_wall_ms_all=[round(t, 2) for t in wall["store"]],
               clashes_list_wall_ms=round(min(wall["list"]), 2), clashes_list_wall_ms_all=[round(t, 2) for t in wall["list"]])

    # (c) the two searches on the same slots
    modes, stride = 4, 8
    hits = np.resize(np.arange(len(dlib)), n // (modes * stride)).astype(np.int64)
    h = len(hits)
    _, _, values, match, _, _, est, _ = _explain_call(model, dlib, hits, modes, None, None, "pmx_explain_modes")
    lib = _ffi.load()
    f64, i32, u8, i64 = torch.float64, torch.int32, torch.uint8, torch.int64
    new = lambda dt, *shape: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
    hl = torch.from_numpy(hits).to(dev)
    mh, ph, w = device_model(model, dlib.device), device_pocket(pocket, dlib.device), _weights_array(None)
    centers = mh.node_centers(model)
    A = dat.max_atoms
    o = dict(choice=new(i32, h, 6), value=new(f64, h, 2), key=new(u8, h, 20), rot=new(f64, h, 9), trans=new(f64, h, 3), fit=new(f64, h, 8), node=new(f64, h, 64),
             count=new(i32, h, 2), levels=new(u8, h, 20), summary=new(f64, h, 4), ccount=new(i32, h, 6), fp=new(i64, h, 4), status=new(i32, h), rs=new(i32, 3, h))
    ppen_n, patom_n = new(f64, h, 64), new(i32, h, 64)
    poff, ppen_a, patom_a = new(i64, h + 1), new(f64, max(h * A, 1)), new(i32, max(h * A, 1))
    need_n, need_a = int(lib.pmx_pose_search_work_bytes(h, modes, stride)), int(lib.pmx_pose_search_atoms_work_bytes(h, modes, stride, A))
    work = new(u8, max(need_n, need_a))
    p = {k: v.data_ptr() for k, v in o.items()}
    head = (centers.data_ptr(), ph.handle, hl.data_ptr(), h, values.data_ptr(), match.data_ptr(), est.data_ptr(), modes, stride, 1.0, 0.5, 4.5, 0, 1, 0.0, p["choice"], p["value"],
            p["key"], p["rot"], p["trans"], p["fit"], p["node"], p["count"], p["levels"], p["summary"], p["ccount"])

    def search_nodes():
        _ffi.check(lib.pmx_pose_search(mh.handle, dlib.handle, w, *head, ppen_n.data_ptr(), patom_n.data_ptr(), p["fp"], p["status"], p["rs"], work.data_ptr(), need_n, stream))

    def search_atoms():
        _ffi.check(lib.pmx_pose_search_atoms(mh.handle, dlib.handle, dat.handle, w, *head, poff.data_ptr(), ppen_a.data_ptr(), patom_a.data_ptr(), p["fp"], p["status"], p["rs"],
                                             work.data_ptr(), need_a, stream))

    out.update(search_hits=h, search_slots=h * modes * stride, search_work_bytes_nodes=need_n, search_work_bytes_atoms=need_a)
    out["search_nodes_device_ms"], out["search_nodes_device_ms_all"] = device_ms(search_nodes)
    out["search_nodes_passing"] = int(o["choice"].cpu().numpy()[:, 2].sum())
    out["search_atoms_device_ms"], out["search_atoms_device_ms_all"] = device_ms(search_atoms)
    out["search_atoms_passing"] = int(o["choice"].cpu().numpy()[:, 2].sum())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
