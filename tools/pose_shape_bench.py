#!/usr/bin/env python3
"""What comparing a pose with a known ligand costs next to checking it against the protein: `pmx_pose_shape` and `pmx_pose_clash` in point
mode over the same atom-store rows (`pmx_atoms_gather`, once, outside the timing) and the same motions - the bench generator's molecules
at their fitted poses, the crystal ligand and the 6OIM pocket of tests/golden.

    python tools/pose_shape_bench.py [--ligands 1024] [--rows 65536] [--repeat 5]

`--ligands` ligands are generated, explained and fitted (`pmx_align`) once; the rows are the OK ones at their best conformer under the
fit's own motion, repeated in order up to `--rows`. Device times between HIP events on the current stream, warm, best and all of
`--repeat` calls. Prints one JSON line."""
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
    ap.add_argument("--ligands", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    import torch

    from conftest import GOLDEN, load_golden
    from pharmaconet_amd import _ffi
    from pharmaconet_amd.atoms import PackedAtoms
    from pharmaconet_amd.engine import DeviceAtoms, DeviceLibrary, device_pocket, device_shape_ref, explain
    from pharmaconet_amd.pocket import PocketAtoms
    from pharmaconet_amd.shape import ReferenceLigand
    from test_survey_library import _model_nodes
    from tools.synthetic import synthetic_library

    model, _, _, _ = load_golden("set_6oim_c8")
    mols = []
    packed = synthetic_library(a.ligands, model_nodes=_model_nodes(model), molecules_out=mols)
    store = PackedAtoms.for_library(mols, packed)
    dlib, dat = DeviceLibrary(packed), DeviceAtoms(store)
    pocket = PocketAtoms.from_pdb(GOLDEN / "pocket_6oim.pdb", centers=model.node_centers)
    reference = ReferenceLigand.from_pdb(GOLDEN / "ligand_6oim_mov.pdb")
    al = explain(model, dlib, np.arange(len(dlib))).poses(model, dlib)
    ok = np.flatnonzero(al.status == 0)
    take = ok[np.resize(np.arange(len(ok)), a.rows)]
    idx, conf = al.indices[take].astype(np.int64), np.asarray(al.conformers)[take].astype(np.int32)
    n = len(idx)

    lib = _ffi.load()
    dev = torch.device("cuda", dlib.device)
    f64, i32 = torch.float64, torch.int32
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    new = lambda dt, *shape: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
    rot, trans = up(al.rotation[take].reshape(n, 9)), up(al.translation[take])
    off, pts, rad, gstatus = dat.gather_device(up(idx), up(conf), n)
    slots = max(n * dat.max_atoms, 1)
    ph, rh = device_pocket(pocket, dlib.device), device_shape_ref(reference, dlib.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    csum, ccnt, ppen, patom, fp, cst = new(f64, n, 4), new(i32, n, 6), new(f64, slots), new(i32, slots), new(torch.int64, n, 4), new(i32, n)
    ssum, scnt, pnear, pref, rnear, rpoint, sst = new(f64, n, 10), new(i32, n, 4), new(f64, slots), new(i32, slots), new(f64, n, 256), new(i32, n, 256), new(i32, n)

    def clash():
        return lib.pmx_pose_clash(ph.handle, None, None, None, off.data_ptr(), pts.data_ptr(), rad.data_ptr(), rot.data_ptr(), trans.data_ptr(), n, 1.0, 0.5, 4.5, csum.data_ptr(),
                                  ccnt.data_ptr(), ppen.data_ptr(), patom.data_ptr(), fp.data_ptr(), cst.data_ptr(), stream)

    def shape():
        return lib.pmx_pose_shape(rh.handle, None, None, None, off.data_ptr(), pts.data_ptr(), rad.data_ptr(), rot.data_ptr(), trans.data_ptr(), n, 1.0, 2.0, ssum.data_ptr(),
                                  scnt.data_ptr(), pnear.data_ptr(), pref.data_ptr(), rnear.data_ptr(), rpoint.data_ptr(), sst.data_ptr(), stream)

    points = float(store.headers()[idx, 0].mean())
    out = dict(rows=n, ligands=len(dlib), points_per_row=points, reference_atoms=len(reference), pocket_atoms=len(pocket),
               exp_per_row=float((store.headers()[idx, 0] * (len(reference) + store.headers()[idx, 0])).mean()), gather_rows_ok=int((gstatus == 0).sum()))
    for name, call in (("pose_shape", shape), ("pose_clash", clash), ("pose_shape_again", shape)):
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
    sm, st = ssum.cpu().numpy(), sst.cpu().numpy()
    out.update(shape_rows_ok=int((st == 0).sum()), clash_rows_ok=int((cst.cpu().numpy() == 0).sum()), mean_tanimoto=float(sm[st == 0, 3].mean()) if (st == 0).any() else 0.0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
