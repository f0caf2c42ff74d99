"""NumPy restatement of `pmx_combo_overlay` (the comment of include/pmx.h): one row at a time, float64 with every operation rounded. The
iteration is tests/lm_ref.py's `lm_loop` and the shape term tests/overlay_ref.py's `evaluate`, both unchanged; this file supplies the colour
term, the combined objective F = O_AB + colour_weight * C_AB and, through `lm_loop`, the row's `decision_margin`. `variant` is
overlay_ref's: "forward" (the header's order), "reverse" (the same terms summed in the reversed order), "jitter" (forward, each component
of every delta multiplied by 1 +- 2^-52). The three differ by rounding alone; how far their results lie apart is the sensitivity figure S
of tests/test_colour_cpu.py, from which the bars of the GPU tests follow."""

import numpy as np

import colour_ref
import overlay_ref
import shape_ref
from lm_ref import _IU, hidx, lm_loop, net_motion
from overlay_ref import _lane_sum, _running

OK, UNSUPPORTED, KEY_INVALID = 0, 1, 4
MAX_ITER = 64
MAX_ATOMS = 256
MAX_NODES = 64


class TypedRow:
    """What the colour term of a row is made of, widened once: the pair weights and constants depend on no motion."""

    def __init__(self, feat_xyz, feat_mask, weights, radius, nodes, masks):
        self.x = np.asarray(nodes, dtype=np.float32).reshape(-1, 3)
        self.n = len(self.x)
        self.ma = np.asarray(masks, dtype=np.int64).reshape(-1)
        self.y = np.asarray(feat_xyz, dtype=np.float32).reshape(-1, 3).astype(np.float64)
        self.mb = np.asarray(feat_mask, dtype=np.int64).reshape(-1)
        assert len(self.ma) == self.n and len(self.mb) == len(self.y)
        self.w = colour_ref.weight_table(weights)[self.ma[:, None] & self.mb[None, :]]
        al = colour_ref.alpha_c(radius)
        s = al + al
        q = shape_ref.PI / s
        self.k = (al * al) / s
        self.pref = 8.0 * (q * np.sqrt(q))


def colour_terms(trow, R, t, c, variant="forward", want_normal=True):
    """C_AB and - `want_normal` - the 21 + 6 values of H_colour and g_colour at (R, t), r taken from c."""
    rev = variant == "reverse"
    p = shape_ref.pose(trow.x, R, t)
    n = trow.n
    e = p[:, None, :] - trow.y[None, :, :]
    d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    with np.errstate(under="ignore"):
        V = np.where(trow.w != 0.0, trow.w * (trow.pref * np.exp(-(trow.k * d2))), 0.0)  # (a pair of weight 0 is left out: + 0.0)
        kappa = (2.0 * trow.k) * V
        acc = _running(np.stack([V, kappa * e[..., 0], kappa * e[..., 1], kappa * e[..., 2], kappa], axis=2), rev)
    cross, f, w = acc[:, 0], acc[:, 1:4], acc[:, 4]
    cab = float(_lane_sum(cross, rev))
    if not want_normal:
        return cab, None
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
    return cab, _lane_sum(at, rev)


def evaluate(row, trow, cw, R, t, variant="forward", want_normal=True):
    """O_AB, C_AB, F, c and - `want_normal` - H (21) and g (6) at (R, t): H = H_shape + cw * H_colour and g likewise, value by value."""
    s = overlay_ref.evaluate(row, R, t, variant, want_normal)
    cab, total = colour_terms(trow, R, t, s["c"], variant, want_normal)
    out = dict(oab=s["oab"], cab=cab, F=float(np.float64(s["oab"]) + np.float64(cw) * np.float64(cab)), c=s["c"])
    if want_normal:
        out["H"] = s["H"] + cw * total[:21]
        out["g"] = s["g"] + cw * total[21:]
    return out


def objective(row, trow, cw, R, t, variant="forward"):
    return evaluate(row, trow, cw, R, t, variant, want_normal=False)["F"]


def normal_equations(row, trow, cw, R, t, variant="forward"):
    """(H [6, 6], g [6], c [3]) at (R, t)."""
    ev = evaluate(row, trow, cw, R, t, variant)
    H = np.zeros((6, 6))
    for k, (i, j) in enumerate(_IU):
        H[i, j] = H[j, i] = ev["H"][k]
    return H, ev["g"], ev["c"]


def colour_self(trow, R, t, weights, radius):
    """C_AA of the nodes posed at (R, t): pmx_pose_colour's."""
    if not trow.n:
        return 0.0
    return colour_ref.colour_row(trow.x, trow.ma, weights, radius, trow.x, trow.ma, R, t, c_bb=0.0)["sums"][1]


def combo_row(ref_xyz, ref_radius, feat_xyz, feat_mask, weights, radius, points, radii, nodes, masks, R, t, colour_weight, ftol=1e-6, max_iter=32, variant="forward", seed=0,
              status=OK, o_bb=None, c_bb=None, trace=None):
    """One row: the shape points `points` with `radii` (per point, or one float32 for all), the typed `nodes` with `masks`. Returns the
    kernel's fields - rotation, translation, energy (16), count (6), status - and `decision_margin`. `status`: what the row front end says
    of the row before anything is read. `trace`, a list, receives F after every accepted step."""
    assert 0 <= max_iter <= MAX_ITER and ftol >= 0 and colour_weight >= 0
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    x = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    rad = np.broadcast_to(np.asarray(radii, dtype=np.float32), (len(x),)) if np.ndim(radii) == 0 else np.asarray(radii, dtype=np.float32).reshape(-1)
    ma = np.asarray(masks, dtype=np.int64).reshape(-1)
    if status == OK and not (np.isfinite(R).all() and np.isfinite(t).all()):
        status = KEY_INVALID
    if status == OK and (len(x) > MAX_ATOMS or len(ma) > MAX_NODES):
        status = UNSUPPORTED
    if status == OK and ((len(x) and not (np.isfinite(rad) & (rad > 0)).all()) or (ma >= 128).any()):
        status = KEY_INVALID
    if status != OK:
        return dict(status=status, rotation=np.full((3, 3), np.nan), translation=np.full(3, np.nan), energy=np.full(16, np.nan), count=np.array([0, 0, -1, 0, 0, 0]),
                    decision_margin=np.inf)
    if o_bb is None:
        o_bb = shape_ref.self_overlap(ref_xyz, ref_radius)
    if c_bb is None:
        c_bb = colour_ref.self_overlap(feat_xyz, feat_mask, weights, radius)
    row = overlay_ref.Row(ref_xyz, ref_radius, x, rad)
    trow = TypedRow(feat_xyz, feat_mask, weights, radius, nodes, ma)
    cw = float(colour_weight)
    rng = np.random.default_rng(seed)
    oaa = overlay_ref.self_overlap_of(row, R, t)
    caa = colour_self(trow, R, t, weights, radius)
    start = evaluate(row, trow, cw, R, t, variant)
    run = lm_loop(lambda Rt, tt: evaluate(row, trow, cw, Rt, tt, variant), lambda ev: ev["F"], lambda trial, cur: trial > cur, lambda before, after: after - before,
                  start["F"] > 0.0, start, R, t, ftol, max_iter, rng if variant == "jitter" else None, trace)
    end = run["cur"]
    angle, shift = net_motion(run["R"], R, run["accepted"], end["c"], start["c"])
    ts0, ts1 = overlay_ref.tanimoto(start["oab"], oaa, o_bb), overlay_ref.tanimoto(end["oab"], oaa, o_bb)
    tc0, tc1 = colour_ref.tanimoto(start["cab"], caa, c_bb), colour_ref.tanimoto(end["cab"], caa, c_bb)
    return dict(status=OK, rotation=run["R"], translation=run["t"],
                energy=np.array([start["oab"], end["oab"], oaa, o_bb, ts0, ts1, start["cab"], end["cab"], caa, c_bb, tc0, tc1, ts0 + tc0, ts1 + tc1, angle, shift]),
                count=np.array([run["iterations"], run["accepted"], run["reason"], row.n, trow.n, len(trow.y)]), F=(start["F"], end["F"]), decision_margin=run["decision_margin"])
