#!/usr/bin/env python3
"""What a shape overlay costs next to the comparison it contains: `pmx_shape_overlay` at `max_iter` 0 and 32 and `pmx_pose_shape` - the
yardstick - in point mode over the rows of tools/pose_shape_bench.py (the bench generator's molecules from the atom store, gathered once
outside the timing, at their fitted poses, against the crystal ligand of tests/golden), and the `starts=4` pipeline (`pmx_shape_starts`,
then `pmx_shape_overlay` from those motions) on a quarter as many hits.

    python tools/shape_overlay_bench.py [--ligands 1024] [--rows 65536] [--repeat 7]

Device times between HIP events on the current stream, warm, best and all of `--repeat` calls. `quotient` is the overlay's time over what
its evaluations would cost at the yardstick's price per pair: shape time x (evaluations + 1) x m / (m + points) - an evaluation walks
points x m pairs where the comparison walks points x (m + points); the + 1 is O_AA, once. Prints one JSON line."""
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
    ap.add_argument("--repeat", type=int, default=7)
    a = ap.parse_args()
    import torch

    from conftest import GOLDEN, load_golden
    from pharmaconet_amd import _ffi
    from pharmaconet_amd.atoms import PackedAtoms
    from pharmaconet_amd.engine import DeviceAtoms, DeviceLibrary, device_shape_ref, explain
    from pharmaconet_amd.shape import ReferenceLigand
    from test_survey_library import _model_nodes
    from tools.synthetic import synthetic_library

    model, _, _, _ = load_golden("set_6oim_c8")
    mols = []
    packed = synthetic_library(a.ligands, model_nodes=_model_nodes(model), molecules_out=mols)
    store = PackedAtoms.for_library(mols, packed)
    dlib, dat = DeviceLibrary(packed), DeviceAtoms(store)
    reference = ReferenceLigand.from_pdb(GOLDEN / "ligand_6oim_mov.pdb")
    al = explain(model, dlib, np.arange(len(dlib))).poses(model, dlib)
    ok = np.flatnonzero(al.status == 0)
    take = ok[np.resize(np.arange(len(ok)), a.rows)]
    idx, conf = al.indices[take].astype(np.int64), np.asarray(al.conformers)[take].astype(np.int32)
    n, m = len(idx), len(reference)
    hits = n // 4  # the starts=4 pipeline: each hit four times, start 0 .. 3

    lib = _ffi.load()
    dev = torch.device("cuda", dlib.device)
    f64, i32 = torch.float64, torch.int32
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    new = lambda dt, *shape: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
    rot, trans = up(al.rotation[take].reshape(n, 9)), up(al.translation[take])
    off, pts, rad, gstatus = dat.gather_device(up(idx), up(conf), n)
    off4, pts4, rad4, _ = dat.gather_device(up(np.repeat(idx[:hits], 4)), up(np.repeat(conf[:hits], 4)), hits * 4)
    which = up((np.arange(hits * 4) % 4).astype(np.int32))
    slots = max(n * dat.max_atoms, 1)
    rh = device_shape_ref(reference, dlib.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ssum, scnt, pnear, pref, rnear, rpoint, sst = new(f64, n, 10), new(i32, n, 4), new(f64, slots), new(i32, slots), new(f64, n, 256), new(i32, n, 256), new(i32, n)
    orot, otrans, oen, ocnt, ost = new(f64, n, 9), new(f64, n, 3), new(f64, n, 8), new(i32, n, 4), new(i32, n)
    srot, strans, frame, sst4 = new(f64, n, 9), new(f64, n, 3), new(f64, n, 16), new(i32, n)

    def shape():
        return lib.pmx_pose_shape(rh.handle, None, None, None, off.data_ptr(), pts.data_ptr(), rad.data_ptr(), rot.data_ptr(), trans.data_ptr(), n, 1.0, 2.0, ssum.data_ptr(),
                                  scnt.data_ptr(), pnear.data_ptr(), pref.data_ptr(), rnear.data_ptr(), rpoint.data_ptr(), sst.data_ptr(), stream)

    def overlay(max_iter, source=None, motion=None, rows=None):
        o, p, r = source or (off, pts, rad)
        R, t = motion or (rot, trans)
        return lib.pmx_shape_overlay(rh.handle, None, None, None, o.data_ptr(), p.data_ptr(), r.data_ptr(), R.data_ptr(), t.data_ptr(), rows or n, 1.0, 1e-6, max_iter, orot.data_ptr(),
                                     otrans.data_ptr(), oen.data_ptr(), ocnt.data_ptr(), ost.data_ptr(), stream)

    def four():
        rc = lib.pmx_shape_starts(rh.handle, None, None, None, off4.data_ptr(), pts4.data_ptr(), which.data_ptr(), hits * 4, srot.data_ptr(), strans.data_ptr(), frame.data_ptr(),
                                  sst4.data_ptr(), stream)
        return rc or overlay(32, (off4, pts4, rad4), (srot, strans), hits * 4)

    npts = store.headers()[idx, 0].astype(np.float64)
    out = dict(rows=n, ligands=len(dlib), points_per_row=float(npts.mean()), reference_atoms=m, gather_rows_ok=int((gstatus == 0).sum()))
    kept = {}
    for name, call in (("pose_shape", shape), ("overlay_iter0", lambda: overlay(0)), ("overlay_iter32", lambda: overlay(32)), ("starts4", four), ("pose_shape_again", shape)):
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
        kept[name] = (oen.cpu().numpy().copy(), ocnt.cpu().numpy().copy(), ost.cpu().numpy().copy())
    shape_ms = min(out["pose_shape_device_ms"], out["pose_shape_again_device_ms"])
    share = float((m / (m + npts)).mean())  # the part of the comparison's pairs that an evaluation walks
    en, cn, st = kept["overlay_iter32"]
    good = st == 0
    evals = float(cn[good, 0].mean())
    out.update(overlay_rows_ok=int(good.sum()), mean_evaluations=evals, stops={str(k): int((cn[good, 2] == k).sum()) for k in range(4)},
               mean_tanimoto_start=float(en[good, 4].mean()), mean_tanimoto=float(en[good, 5].mean()), mean_shift=float(en[good, 7].mean()),
               mean_angle_deg=float(np.degrees(en[good, 6]).mean()), pair_share=share,
               quotient_iter0=out["overlay_iter0_device_ms"] / (shape_ms * share), quotient_iter32=out["overlay_iter32_device_ms"] / ((evals + 1.0) * shape_ms * share))
    en4, cn4, st4 = (v[: hits * 4] for v in kept["starts4"])
    each = np.where(st4 == 0, en4[:, 5], -np.inf).reshape(hits, 4)
    local = np.where(good[:hits], en[:hits, 5], -np.inf)  # the same hits from their fitted poses (the first `hits` rows)
    both = np.isfinite(each.max(axis=1)) & np.isfinite(local)
    out.update(starts4_hits=hits, starts4_mean_evaluations=float(cn4[st4 == 0, 0].mean()), starts4_mean_best_tanimoto=float(each.max(axis=1)[both].mean()),
               starts4_kept={str(k): int((np.argmax(each, axis=1)[both] == k).sum()) for k in range(4)},
               starts4_beats_fitted_pose=float((each.max(axis=1)[both] > local[both]).mean()), fitted_pose_mean_tanimoto_same_hits=float(local[both].mean()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
