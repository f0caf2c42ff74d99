"""NumPy restatement of `pmx_pose_clash` (the comment of include/pmx.h): one row at a time, float64 with every operation rounded in the
order the header gives. NumPy's `a * b + c` on float64 arrays is two rounded operations (no fused multiply-add), `np.sqrt` is correctly
rounded. The overlap is summed here by NumPy's pairwise sum over the pairs in (point, atom) order; the kernel's order differs, hence the relative bar of the GPU tests."""

import numpy as np

OK, UNSUPPORTED, KEY_INVALID = 0, 1, 4
WORDS = 4


def pose(points, R, t):
    """float32 [m, 3] points under (R, t): p_k = ((R[k][0] x_0 + R[k][1] x_1) + R[k][2] x_2) + t_k."""
    x = np.asarray(points, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    return np.stack([((R[k, 0] * x[:, 0] + R[k, 1] * x[:, 1]) + R[k, 2] * x[:, 2]) + t[k] for k in range(3)], axis=1)


def clash_row(atom_xyz, atom_radius, atom_group, points, radii, R, t, tolerance=0.5, contact=4.5):
    """One row: `points` float32 [m, 3], `radii` float32 [m] (or a scalar). Returns a dict with summary (clearance, overlap), the six counts,
    point_pen / point_atom, the contact fingerprint (uint64 [4]), status and `margin`: the smallest |pen| and |d - contact| over all pairs
    (inf without a pair) - how far the row's integers are from changing."""
    pts = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    m = len(pts)
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    if not (np.isfinite(R).all() and np.isfinite(t).all()):
        return dict(status=KEY_INVALID, clearance=np.nan, overlap=np.nan, counts=np.array([0, 0, 0, 0, -1, -1]), point_pen=np.full(m, np.nan),
                    point_atom=np.full(m, -1), fingerprint=np.zeros(WORDS, np.uint64), margin=np.inf)
    y = np.asarray(atom_xyz, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    ra = np.asarray(atom_radius, dtype=np.float32).reshape(-1).astype(np.float64)
    na = len(y)
    group = np.full(na, 0xFFFF, np.uint16) if atom_group is None else np.asarray(atom_group, dtype=np.uint16).reshape(-1)
    rp = np.broadcast_to(np.asarray(radii, dtype=np.float32), (m,)).astype(np.float64)
    tol, con = float(np.float32(tolerance)), float(np.float32(contact))
    p = pose(pts, R, t)
    dx, dy, dz = (p[:, None, k] - y[None, :, k] for k in range(3))
    d = np.sqrt((dx * dx + dy * dy) + dz * dz)  # [m, na]
    s = (ra[None, :] + rp[:, None]) - tol
    pen = s - d
    clash, touch = pen > 0, d < con
    point_pen = pen.max(axis=1) if na else np.full(m, -np.inf)
    point_atom = pen.argmax(axis=1) if na else np.full(m, -1)  # (argmax: the first among equals)
    if m and na:
        wp = int(point_pen.argmax())
        clearance, worst = float(point_pen[wp]), (wp, int(point_atom[wp]))
    else:
        clearance, worst = -np.inf, (-1, -1)
    overlap = float(np.sum(pen[clash] ** 2)) if m and na else 0.0
    bits = np.zeros(256, np.uint8)
    touched = np.flatnonzero(touch.any(axis=0)) if m else np.zeros(0, np.int64)
    g = group[touched]
    bits[g[g < 256]] = 1
    fp = np.packbits(bits, bitorder="little").view(np.uint64).copy()
    margin = float(min(np.abs(pen).min(), np.abs(d - con).min())) if m and na else np.inf
    counts = np.array([m, int(clash.any(axis=1).sum()), int(clash.sum()), int(touch.any(axis=1).sum()), worst[0], worst[1]])
    return dict(status=OK, clearance=clearance, overlap=overlap, counts=counts, point_pen=point_pen, point_atom=np.asarray(point_atom, dtype=np.int64),
                fingerprint=fp, margin=margin)
