#!/usr/bin/env python3
"""What the colour term costs: `pmx_combo_overlay` next to `pmx_shape_overlay` on the same rows - the hits of a golden set (tests/golden) with
their heavy atoms from the atom store as the shape points and their pharmacophore nodes as the typed points, at their fitted poses, tiled
to `--rows` rows, against the set's best hit as the known ligand (`ReferenceLigand.from_library`: its atoms and its features) - and
`pmx_pose_colour` on those rows.

    python tools/colour_bench.py [--rows 4096] [--repeat 9] [--set set_6oim_c8]

Device times between HIP events on the current stream. The atoms are gathered once, outside the timing. After one warm-up of each call the
two overlays are timed in turn, `--repeat` times each, so that what else the machine does meets both; the best and all times are printed,
and `combo_over_shape`, the ratio of the two best. The colour term adds at most 64 x 64 pairs and 20 butterflies to an evaluation of up to
256 x 256 pairs. Prints one JSON line."""
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
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--repeat", type=int, default=9)
    ap.add_argument("--set", type=str, default="set_6oim_c8")
    a = ap.parse_args()
    import torch

    from conftest import load_golden
    from pharmaconet_amd import _ffi
    from pharmaconet_amd.atoms import PackedAtoms
    from pharmaconet_amd.engine import DeviceAtoms, DeviceLibrary, device_colour_ref, device_shape_ref, explain
    from pharmaconet_amd.shape import ReferenceLigand
    from test_attribution_cpu import load_mols

    model, packed, _, _ = load_golden(a.set)
    store = PackedAtoms.for_library(load_mols(a.set), packed)
    dlib, dat = DeviceLibrary(packed), DeviceAtoms(store)
    res = model.screen(dlib)
    al = explain(model, dlib, np.arange(len(dlib))).poses(model, dlib)
    ok = np.flatnonzero(al.status == 0)
    best = int(ok[np.argmax(res.scores.cpu().numpy()[al.indices[ok]])])
    reference = ReferenceLigand.from_library(packed, int(al.indices[best]), int(al.conformers[best]), atoms=store, rotation=al.rotation[best], translation=al.translation[best])
    take = ok[np.resize(np.arange(len(ok)), a.rows)]
    idx, conf = al.indices[take].astype(np.int64), np.asarray(al.conformers)[take].astype(np.int32)
    n = len(idx)

    lib = _ffi.load()
    dev = torch.device("cuda", dlib.device)
    f64, i32 = torch.float64, torch.int32
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    new = lambda dt, *shape: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
    t_idx, t_conf, rot, trans = up(idx), up(conf), up(al.rotation[take].reshape(n, 9)), up(al.translation[take])
    off, pts, rad, gstatus = dat.gather_device(t_idx, t_conf, n)
    sh, co = device_shape_ref(reference, dlib.device), device_colour_ref(reference, dlib.device)
    cw = sh.self_overlap / co.self_overlap
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    orot, otrans, oen, ocnt, ost = new(f64, n, 9), new(f64, n, 3), new(f64, n, 16), new(i32, n, 6), new(i32, n)
    sen, scnt = new(f64, n, 8), new(i32, n, 4)  # (pmx_shape_overlay's energy and count)
    csum, ctyp, ccnt, cfp = new(f64, n, 8), new(f64, n, 7), new(i32, n, 4), new(torch.int64, n, 4)
    cn1, cn2, cn3, cf1, cf2 = new(f64, n, 64), new(f64, n, 64), new(i32, n, 64), new(f64, n, 64), new(i32, n, 64)

    def shape_overlay():
        return lib.pmx_shape_overlay(sh.handle, None, None, None, off.data_ptr(), pts.data_ptr(), rad.data_ptr(), rot.data_ptr(), trans.data_ptr(), n, 1.0, 1e-6, 32, orot.data_ptr(),
                                     otrans.data_ptr(), sen.data_ptr(), scnt.data_ptr(), ost.data_ptr(), stream)

    def combo_overlay(weight=cw):
        return lib.pmx_combo_overlay(sh.handle, co.handle, dlib.handle, t_idx.data_ptr(), t_conf.data_ptr(), off.data_ptr(), pts.data_ptr(), rad.data_ptr(), rot.data_ptr(),
                                     trans.data_ptr(), n, 1.0, weight, 1e-6, 32, orot.data_ptr(), otrans.data_ptr(), oen.data_ptr(), ocnt.data_ptr(), ost.data_ptr(), stream)

    def pose_colour():
        return lib.pmx_pose_colour(co.handle, dlib.handle, t_idx.data_ptr(), t_conf.data_ptr(), None, None, None, rot.data_ptr(), trans.data_ptr(), n, 2.0, csum.data_ptr(), ctyp.data_ptr(),
                                   ccnt.data_ptr(), cn1.data_ptr(), cn2.data_ptr(), cn3.data_ptr(), cf1.data_ptr(), cf2.data_ptr(), cfp.data_ptr(), ost.data_ptr(), stream)

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _ffi.check(call())
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    calls = dict(shape_overlay=shape_overlay, combo_overlay=combo_overlay, combo_overlay_weight0=lambda: combo_overlay(0.0), pose_colour=pose_colour)
    times = {name: [] for name in calls}
    kept = {}
    for name, call in calls.items():  # (the warm-up, and what each call returns)
        timed(call)
        kept[name] = ((sen if name == "shape_overlay" else oen).cpu().numpy().copy(), (scnt if name == "shape_overlay" else ocnt).cpu().numpy().copy(), ost.cpu().numpy().copy())
    for _ in range(a.repeat):
        for name, call in calls.items():
            times[name].append(timed(call))
    heads = packed.headers()
    out = dict(set=a.set, rows=n, ligands=len(dlib), shape_points_per_row=float(store.headers()[idx, 0].mean()), nodes_per_row=float(heads[idx, 0].mean()),
               reference_atoms=len(reference), reference_features=len(reference.colour), colour_weight=cw, gather_rows_ok=int((gstatus == 0).sum()))
    for name in calls:
        out[f"{name}_device_ms"] = round(min(times[name]), 3)
        out[f"{name}_device_ms_all"] = [round(t, 3) for t in times[name]]
    out["combo_over_shape"] = out["combo_overlay_device_ms"] / out["shape_overlay_device_ms"]
    out["combo_weight0_over_shape"] = out["combo_overlay_weight0_device_ms"] / out["shape_overlay_device_ms"]
    en_s, cn_s, st_s = kept["shape_overlay"]
    en_c, cn_c, st_c = kept["combo_overlay"]
    en_0, cn_0, _ = kept["combo_overlay_weight0"]
    good = (st_s == 0) & (st_c == 0)
    out.update(rows_ok=int(good.sum()), shape_mean_evaluations=float(cn_s[good, 0].mean()), combo_mean_evaluations=float(cn_c[good, 0].mean()),
               weight0_has_the_shape_overlays_bits=bool(np.array_equal(en_0[good, :6], en_s[good, :6]) and np.array_equal(cn_0[good, :4], cn_s[good, :4])),
               mean_shape_tanimoto_after_shape_overlay=float(en_s[good, 5].mean()), mean_shape_tanimoto_after_combo=float(en_c[good, 5].mean()),
               mean_colour_tanimoto_start=float(en_c[good, 10].mean()), mean_colour_tanimoto_after_combo=float(en_c[good, 11].mean()),
               mean_colour_tanimoto_after_shape_overlay=float(en_0[good, 11].mean()), mean_combo_after_combo=float(en_c[good, 13].mean()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
