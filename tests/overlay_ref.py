"""NumPy restatement of `pmx_shape_overlay` and `pmx_shape_starts` (the comment of include/pmx.h): one row at a time, float64 with every
operation rounded (NumPy's `a * b + c` on float64 is two rounded operations). `variant` says how the sums c, cross, f, w, O_AB, H and g are
taken and how the step is applied:

  "forward"   the header's order: a point's terms in ascending atom, a lane's points (point % 64) ascending, the fixed xor butterfly
  "reverse"   the same terms, summed one after the other in the reversed order
  "jitter"    forward, with each component of every delta multiplied by 1 +- 2^-52 from a seeded generator

The three differ by rounding alone; how far their results lie apart is the sensitivity figure S of tests/test_overlay_cpu.py, from which the
bars of the GPU tests follow. The iteration itself is tests/lm_ref.py's, which the refinement's restatement runs too; `overlay_row` also
returns its `decision_margin` - how far the row's integers are from changing.

The frame and the starts use only + - * / and sqrt, one Python float at a time: the device has the same bits."""

import math

import numpy as np

import shape_ref
from lm_ref import _IU, LANES, _butterfly, hidx, lm_loop, net_motion

OK, UNSUPPORTED, KEY_INVALID = 0, 1, 4
MAX_ITER = 64
MAX_ATOMS = 256
JACOBI_SWEEPS = 8


def _lane_sum(terms, reverse=False):
    """The sum of terms[k] (shape [n] or [n, w]), term k in lane k % 64, a lane's terms ascending from 0.0, then the butterfly; `reverse`:
    one after the other from the last."""
    terms = np.asarray(terms, dtype=np.float64)
    width = terms.shape[1:]
    if reverse:
        return np.cumsum(terms[::-1], axis=0)[-1] if len(terms) else np.zeros(width)
    lanes = np.zeros((LANES,) + width)
    for base in range(0, len(terms), LANES):
        part = terms[base: base + LANES]
        lanes[: len(part)] = lanes[: len(part)] + part
    return _butterfly(lanes)


def _running(terms, reverse=False):
    """terms [n, m, w] summed over axis 1 one after the other, from 0.0 (cumsum adds one term at a time)."""
    if reverse:
        terms = terms[:, ::-1]
    zero = np.zeros((terms.shape[0], 1) + terms.shape[2:])
    return np.cumsum(np.concatenate([zero, terms], axis=1), axis=1)[:, -1]


class Row:
    """What a row is made of, widened once: the pair constants depend on no motion."""

    def __init__(self, ref_xyz, ref_radius, points, radii):
        self.x = np.asarray(points, dtype=np.float32).reshape(-1, 3)
        self.n = len(self.x)
        self.y = np.asarray(ref_xyz, dtype=np.float32).reshape(-1, 3).astype(np.float64)
        self.ab = shape_ref.alpha(ref_radius)
        rad = np.broadcast_to(np.asarray(radii, dtype=np.float32), (self.n,)) if np.ndim(radii) == 0 else np.asarray(radii, dtype=np.float32).reshape(-1)
        assert len(rad) == self.n
        self.rad = rad
        with np.errstate(all="ignore"):
            self.aa = shape_ref.alpha(rad)
            s = self.aa[:, None] + self.ab[None, :]
            q = shape_ref.PI / s
            self.k = (self.aa[:, None] * self.ab[None, :]) / s
            self.pref = 8.0 * (q * np.sqrt(q))


def evaluate(row, R, t, variant="forward", want_normal=True):
    """O_AB, c, H (21), g (6) at (R, t)."""
    rev = variant == "reverse"
    p = shape_ref.pose(row.x, R, t)
    n = row.n
    c = _lane_sum(p, rev) / float(n) if n else np.zeros(3)
    e = p[:, None, :] - row.y[None, :, :]
    d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    V = row.pref * np.exp(-(row.k * d2))
    kappa = (2.0 * row.k) * V
    acc = _running(np.stack([V, kappa * e[..., 0], kappa * e[..., 1], kappa * e[..., 2], kappa], axis=2), rev)
    cross, f, w = acc[:, 0], acc[:, 1:4], acc[:, 4]
    oab = float(_lane_sum(cross, rev))
    if not want_normal:
        return dict(oab=oab, c=c)
    r = p - c
    rr = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
    at = np.zeros((n, 27))
    at[:, hidx(0, 0)] = w * (rr - r[:, 0] * r[:, 0])
    at[:, hidx(0, 1)] = w * -(r[:, 0] * r[:, 1])
    at[:, hidx(0, 2)] = w * -(r[:, 0] * r[:, 2])
    at[:, hidx(1, 1)] = w * (rr - r[:, 1] * r[:, 1])
    at[:, hidx(1, 2)] = w * -(r[:, 1] * r[:, 2])
    at[:, hidx(2, 2)] = w * (rr - r[:, 2] * r[:, 2])
    at[:, hidx(0, 4)] = w * -r[:, 2]
    at[:, hidx(0, 5)] = w * r[:, 1]
    at[:, hidx(1, 3)] = w * r[:, 2]
    at[:, hidx(1, 5)] = w * -r[:, 0]
    at[:, hidx(2, 3)] = w * -r[:, 1]
    at[:, hidx(2, 4)] = w * r[:, 0]
    at[:, hidx(3, 3)] = at[:, hidx(4, 4)] = at[:, hidx(5, 5)] = w
    at[:, 21] = r[:, 1] * f[:, 2] - r[:, 2] * f[:, 1]
    at[:, 22] = r[:, 2] * f[:, 0] - r[:, 0] * f[:, 2]
    at[:, 23] = r[:, 0] * f[:, 1] - r[:, 1] * f[:, 0]
    at[:, 24:27] = f
    total = _lane_sum(at, rev)
    return dict(oab=oab, c=c, H=total[:21].copy(), g=total[21:].copy())


def overlap(row, R, t, variant="forward"):
    return evaluate(row, R, t, variant, want_normal=False)["oab"]


def normal_equations(row, R, t, variant="forward"):
    """(H [6, 6], g [6], c [3]) at (R, t)."""
    ev = evaluate(row, R, t, variant)
    H = np.zeros((6, 6))
    for k, (i, j) in enumerate(_IU):
        H[i, j] = H[j, i] = ev["H"][k]
    return H, ev["g"], ev["c"]


def self_overlap_of(row, R, t):
    """O_AA of the points posed at (R, t), in pmx_pose_shape's order."""
    p = shape_ref.pose(row.x, R, t)
    if not row.n:
        return 0.0
    e = p[:, None, :] - p[None, :, :]
    d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    selfs = _running(shape_ref.pair_terms(d2, row.aa[:, None], row.aa[None, :])[:, :, None])[:, 0]
    return shape_ref.lane_sum(selfs)


def tanimoto(oab, oaa, obb):
    with np.errstate(all="ignore"):
        return float(np.float64(oab) / ((np.float64(oaa) + np.float64(obb)) - np.float64(oab)))


def overlay_row(ref_xyz, ref_radius, points, radii, R, t, ftol=1e-6, max_iter=32, variant="forward", seed=0, status=OK, o_bb=None, trace=None):
    """One row. Returns the kernel's fields - rotation, translation, energy (8), count (4), status - and `decision_margin`. `status`: what
    the row front end says of a node-mode row before anything is read. `trace`, a list, receives O_AB after every accepted step."""
    assert 0 <= max_iter <= MAX_ITER and ftol >= 0
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    x = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    rad = np.broadcast_to(np.asarray(radii, dtype=np.float32), (len(x),)) if np.ndim(radii) == 0 else np.asarray(radii, dtype=np.float32).reshape(-1)
    if status == OK and not (np.isfinite(R).all() and np.isfinite(t).all()):
        status = KEY_INVALID
    if status == OK and len(x) > MAX_ATOMS:
        status = UNSUPPORTED
    if status == OK and len(x) and not (np.isfinite(rad) & (rad > 0)).all():
        status = KEY_INVALID
    if status != OK:
        return dict(status=status, rotation=np.full((3, 3), np.nan), translation=np.full(3, np.nan), energy=np.full(8, np.nan), count=np.array([0, 0, -1, 0]), decision_margin=np.inf)
    if o_bb is None:
        o_bb = shape_ref.self_overlap(ref_xyz, ref_radius)
    row = Row(ref_xyz, ref_radius, x, rad)
    rng = np.random.default_rng(seed)
    oaa = self_overlap_of(row, R, t)
    start = evaluate(row, R, t, variant)
    run = lm_loop(lambda Rt, tt: evaluate(row, Rt, tt, variant), lambda ev: ev["oab"], lambda trial, cur: trial > cur, lambda before, after: after - before,
                  row.n != 0 and start["oab"] > 0.0, start, R, t, ftol, max_iter, rng if variant == "jitter" else None, trace)
    O = run["value"]
    angle, shift = net_motion(run["R"], R, run["accepted"], run["cur"]["c"], start["c"])
    return dict(status=OK, rotation=run["R"], translation=run["t"],
                energy=np.array([start["oab"], O, oaa, o_bb, tanimoto(start["oab"], oaa, o_bb), tanimoto(O, oaa, o_bb), angle, shift]),
                count=np.array([run["iterations"], run["accepted"], run["reason"], row.n]), decision_margin=run["decision_margin"])


# ---------------------------------------------------------------------------------------------------------------- frames and starts
def frame(points):
    """(centre [3], axes [3, 3] - axis k is row k -, values [3]) of a point set given as float64 [n, 3]."""
    x = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(x)
    if n < 1:
        return np.zeros(3), np.eye(3), np.zeros(3)
    c = _lane_sum(x) / float(n)
    d = x - c
    S = _lane_sum(np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2], d[:, 2] * d[:, 2]], axis=1))
    S = [float(v) for v in S]
    A = [[S[0], S[1], S[2]], [S[1], S[3], S[4]], [S[2], S[4], S[5]]]
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(JACOBI_SWEEPS):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            r = 3 - p - q
            apq = A[p][q]
            if apq != 0.0:
                app, aqq = A[p][p], A[q][q]
                theta = (aqq - app) / (2.0 * apq)
                at = abs(theta) + math.sqrt(theta * theta + 1.0)
                tn = 1.0 / at if theta >= 0.0 else -1.0 / at
                cc = 1.0 / math.sqrt(tn * tn + 1.0)
                ss = tn * cc
                A[p][p] = app - tn * apq
                A[q][q] = aqq + tn * apq
                A[p][q] = A[q][p] = 0.0
                arp, arq = A[r][p], A[r][q]
                A[r][p] = A[p][r] = cc * arp - ss * arq
                A[r][q] = A[q][r] = ss * arp + cc * arq
                for k in range(3):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = cc * vkp - ss * vkq
                    V[k][q] = ss * vkp + cc * vkq
    ev = [A[0][0], A[1][1], A[2][2]]
    order = sorted(range(3), key=lambda i: -ev[i])  # (stable: equal values keep the lower index)
    ax = np.array([[V[j][order[k]] for j in range(3)] for k in range(3)])
    ax[2] = [ax[0][1] * ax[1][2] - ax[0][2] * ax[1][1], ax[0][2] * ax[1][0] - ax[0][0] * ax[1][2], ax[0][0] * ax[1][1] - ax[0][1] * ax[1][0]]
    return c, ax, np.array([ev[i] for i in order])


SIGNS = ((1.0, 1.0, 1.0), (1.0, -1.0, -1.0), (-1.0, 1.0, -1.0), (-1.0, -1.0, 1.0))


def starts_row(ref_xyz, points, start, status=OK):
    """One row of `pmx_shape_starts`: rotation, translation, frame (16), status."""
    x = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    if status == OK and len(x) > MAX_ATOMS:
        status = UNSUPPORTED
    if status == OK and not 0 <= int(start) <= 3:
        status = KEY_INVALID
    if status != OK:
        return dict(status=status, rotation=np.full((3, 3), np.nan), translation=np.full(3, np.nan), frame=np.full(16, np.nan))
    ca, a, eva = frame(x.astype(np.float64))
    cb, b, _ = frame(np.asarray(ref_xyz, dtype=np.float32).reshape(-1, 3).astype(np.float64))
    d = SIGNS[int(start)]
    R = np.array([[(d[0] * (b[0, i] * a[0, j]) + d[1] * (b[1, i] * a[1, j])) + d[2] * (b[2, i] * a[2, j]) for j in range(3)] for i in range(3)])
    t = np.array([cb[i] - ((R[i, 0] * ca[0] + R[i, 1] * ca[1]) + R[i, 2] * ca[2]) for i in range(3)])
    return dict(status=OK, rotation=R, translation=t, frame=np.concatenate([ca, a.reshape(-1), eva, [0.0]]))
