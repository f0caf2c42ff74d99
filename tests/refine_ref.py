"""NumPy restatement of `pmx_pose_refine` (the comment of include/pmx.h): one row at a time, float64 with every operation rounded (NumPy's
`a * b + c` on float64 is two rounded operations). `variant` says how the sums Ec, Er, c, H and g are taken and how the step is applied:

  "forward"   the header's order: per lane (point % 64, anchor % 64) the terms in ascending order, then the fixed xor butterfly
  "reverse"   the same terms, summed one after the other in the reversed order
  "jitter"    forward, with each component of every delta multiplied by 1 +- 2^-52 from a seeded generator

The three differ by rounding alone; how far their results lie apart is the sensitivity figure S of tests/test_refine_cpu.py, from which the
bars of the GPU tests follow. The iteration itself is tests/lm_ref.py's, which the overlay's restatement runs too; `refine_row` also returns
its `decision_margin` - how far the row's integers are from changing."""

import numpy as np

import clash_ref
from lm_ref import _IU, LANES, _butterfly, _mat3, hidx, lm_loop, net_motion, rodrigues, solve  # noqa: F401 (other test modules take them from here)

OK, UNSUPPORTED, KEY_INVALID = 0, 1, 4
MAX_ITER = 64


def _lane_sum(terms, slots, variant):
    """The sum of terms[k] (shape [m] or [m, w]), term k standing in lane slots[k] % 64, the terms of a lane in the order given."""
    terms = np.asarray(terms, dtype=np.float64)
    width = terms.shape[1:]
    if variant == "reverse":
        return np.cumsum(terms[::-1], axis=0)[-1] if len(terms) else np.zeros(width)  # (cumsum adds one term after the other)
    lanes = np.zeros((LANES,) + width)
    slots = np.asarray(slots, dtype=np.int64)
    if len(terms) and np.array_equal(slots, np.arange(len(terms))):  # (a dense run: a trip of the wave at a time)
        for base in range(0, len(terms), LANES):
            part = terms[base: base + LANES]
            lanes[: len(part)] = lanes[: len(part)] + part
    else:
        for k in range(len(terms)):
            lanes[slots[k] % LANES] = lanes[slots[k] % LANES] + terms[k]
    return _butterfly(lanes)


class Row:
    """What a row is made of, widened once."""

    def __init__(self, atom_xyz, atom_radius, points, radii, anchors=None, targets=None, weights=None, R=None, t=None, tolerance=0.5, restraint=0.1):
        self.x = np.asarray(points, dtype=np.float32).reshape(-1, 3)
        self.m = len(self.x)
        self.y = np.asarray(atom_xyz, dtype=np.float32).reshape(-1, 3).astype(np.float64)
        self.ra = np.asarray(atom_radius, dtype=np.float32).reshape(-1).astype(np.float64)
        self.rp = np.broadcast_to(np.asarray(radii, dtype=np.float32), (self.m,)).astype(np.float64)
        self.tol = float(np.float32(tolerance))
        self.restraint = float(restraint)
        self.R0 = np.asarray(R, dtype=np.float64).reshape(3, 3)
        self.t0 = np.asarray(t, dtype=np.float64).reshape(3)
        self.a = self.x if anchors is None else np.asarray(anchors, dtype=np.float32).reshape(-1, 3)
        self.w = np.ones(len(self.a)) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
        self.b = clash_ref.pose(self.a, self.R0, self.t0) if targets is None else np.asarray(targets, dtype=np.float64).reshape(-1, 3)
        self.s = (self.ra[None, :] + self.rp[:, None]) - self.tol


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def evaluate(row, R, t, variant="forward", want_normal=True):
    """Ec, Er, pairs, c, H (21), g (6) at (R, t)."""
    order = "reverse" if variant == "reverse" else "forward"
    p = clash_ref.pose(row.x, R, t)
    m = row.m
    c = _lane_sum(p, np.arange(m), order) / float(m) if m else np.zeros(3)
    dx, dy, dz = (p[:, None, k] - row.y[None, :, k] for k in range(3))
    d = np.sqrt((dx * dx + dy * dy) + dz * dz)
    pen = row.s - d
    clash = pen > 0
    uj = np.argwhere(clash)  # (point, atom) order
    pairs = len(uj)
    pen_c = pen[clash]
    if order == "forward":
        pov = np.zeros(m)
        for (u, _), v in zip(uj, pen_c):  # a point's pairs in atom order
            pov[u] = pov[u] + v * v
        Ec = float(_lane_sum(pov, np.arange(m), order))
    else:
        Ec = float(_lane_sum(pen_c * pen_c, None, order))
    q = clash_ref.pose(row.a, R, t)
    e = q - row.b
    Er = float(_lane_sum(row.w * ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]), np.arange(len(q)), order))
    if not want_normal:
        return dict(Ec=Ec, Er=Er, pairs=pairs, c=c)
    # pairs: v = [(p - c) x nhat, nhat], H += v v^T, g += -v pen
    keep = d[clash] > 0
    uj, pen_k, dk = uj[keep], pen_c[keep], d[clash][keep]
    r = p[uj[:, 0]] - c
    nh = np.stack([dx[clash][keep] / dk, dy[clash][keep] / dk, dz[clash][keep] / dk], axis=1) if len(uj) else np.zeros((0, 3))
    v = np.concatenate([_cross(r, nh), nh], axis=1) if len(uj) else np.zeros((0, 6))
    pair_terms = np.zeros((len(uj), 27))
    for k, (i, j) in enumerate(_IU):
        pair_terms[:, k] = v[:, i] * v[:, j]
    pair_terms[:, 21:] = -v * pen_k[:, None]
    # anchors: the closed form in r = q - c, k = restraint * w
    r = q - c
    kw = row.restraint * row.w
    rr = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
    at = np.zeros((len(q), 27))
    at[:, hidx(0, 0)] = kw * (rr - r[:, 0] * r[:, 0])
    at[:, hidx(0, 1)] = kw * -(r[:, 0] * r[:, 1])
    at[:, hidx(0, 2)] = kw * -(r[:, 0] * r[:, 2])
    at[:, hidx(1, 1)] = kw * (rr - r[:, 1] * r[:, 1])
    at[:, hidx(1, 2)] = kw * -(r[:, 1] * r[:, 2])
    at[:, hidx(2, 2)] = kw * (rr - r[:, 2] * r[:, 2])
    at[:, hidx(0, 4)] = kw * -r[:, 2]
    at[:, hidx(0, 5)] = kw * r[:, 1]
    at[:, hidx(1, 3)] = kw * r[:, 2]
    at[:, hidx(1, 5)] = kw * -r[:, 0]
    at[:, hidx(2, 3)] = kw * -r[:, 1]
    at[:, hidx(2, 4)] = kw * r[:, 0]
    at[:, hidx(3, 3)] = at[:, hidx(4, 4)] = at[:, hidx(5, 5)] = kw
    at[:, 21:24] = kw[:, None] * _cross(r, e)
    at[:, 24:27] = kw[:, None] * e
    if order == "forward":
        lanes = np.zeros((LANES, 27))
        for k in range(len(uj)):
            lane = uj[k, 0] % LANES
            lanes[lane] = lanes[lane] + pair_terms[k]
        for base in range(0, len(at), LANES):
            part = at[base: base + LANES]
            lanes[: len(part)] = lanes[: len(part)] + part
        total = _butterfly(lanes)
    else:
        total = _lane_sum(np.concatenate([pair_terms, at]), None, order)
    return dict(Ec=Ec, Er=Er, pairs=pairs, c=c, H=total[:21].copy(), g=total[21:].copy())


def energy(row, R, t, variant="forward"):
    ev = evaluate(row, R, t, variant, want_normal=False)
    return ev["Ec"] + row.restraint * ev["Er"]


def normal_equations(row, R, t, variant="forward"):
    """(H [6, 6], g [6], c [3]) at (R, t)."""
    ev = evaluate(row, R, t, variant)
    H = np.zeros((6, 6))
    for k, (i, j) in enumerate(_IU):
        H[i, j] = H[j, i] = ev["H"][k]
    return H, ev["g"], ev["c"]


def refine_row(atom_xyz, atom_radius, points, radii, R, t, anchors=None, targets=None, weights=None, tolerance=0.5, restraint=0.1, ftol=1e-9, max_iter=32,
               variant="forward", seed=0, trace=None):
    """One row. Returns the kernel's fields - rotation, translation, energy (8), count (4), status - and `decision_margin`. `trace`, a
    list, receives E after every accepted step."""
    assert 0 <= max_iter <= MAX_ITER and restraint >= 0 and ftol >= 0
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    bad = dict(status=KEY_INVALID, rotation=np.full((3, 3), np.nan), translation=np.full(3, np.nan), energy=np.full(8, np.nan), count=np.array([0, 0, -1, 0]), decision_margin=np.inf)
    if not (np.isfinite(R).all() and np.isfinite(t).all()):
        return bad
    if weights is not None and not (np.isfinite(np.asarray(weights, dtype=np.float64)).all() and (np.asarray(weights, dtype=np.float64) >= 0).all()):
        return bad
    row = Row(atom_xyz, atom_radius, points, radii, anchors, targets, weights, R, t, tolerance, restraint)
    rng = np.random.default_rng(seed)
    start = evaluate(row, R, t, variant)
    run = lm_loop(lambda Rt, tt: evaluate(row, Rt, tt, variant), lambda ev: ev["Ec"] + row.restraint * ev["Er"], lambda trial, cur: trial < cur,
                  lambda before, after: before - after, start["pairs"] != 0, start, R, t, ftol, max_iter, rng if variant == "jitter" else None, trace)
    cur = run["cur"]
    angle, shift = net_motion(run["R"], row.R0, run["accepted"], cur["c"], start["c"])
    wsum = float(_lane_sum(row.w, np.arange(len(row.w)), "forward")) if anchors is not None else float(row.m)
    rmsd = float(np.sqrt(cur["Er"] / wsum)) if wsum > 0 else 0.0
    return dict(status=OK, rotation=run["R"], translation=run["t"], energy=np.array([start["Ec"], start["Er"], cur["Ec"], cur["Er"], rmsd, angle, shift, run["lam"]]),
                count=np.array([run["iterations"], run["accepted"], run["reason"], cur["pairs"]]), decision_margin=run["decision_margin"])
