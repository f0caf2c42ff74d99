"""NumPy restatement of the Levenberg-Marquardt loop over a row's six rigid degrees of freedom that `pmx_pose_refine` and
`pmx_shape_overlay` share (csrc/pmx_lm.h; the comment of include/pmx.h): the 6x6 solve, Rodrigues, the iteration and the net angle and
centroid shift, float64 with every operation rounded. tests/refine_ref.py and tests/overlay_ref.py supply the objective - `evaluate`, the
value that is followed, which of two values is better and what a step gained - and keep their rows, statuses and output layout.

`lm_loop` also returns `decision_margin`: the smallest relative distance of any decision the row took from its threshold - |E' - E| / E
of every accept or reject (but 0 against 0, which is no matter of rounding), |gain - ftol E| / E of every accepted step, |lambda - 1e8| /
1e8 of every rejected one - which says how far the row's integers are from changing."""

import numpy as np

LANES = 64
_XOR = [np.arange(LANES) ^ m for m in (1, 2, 4, 8, 16, 32)]


def hidx(i, j):
    return i * 6 - i * (i - 1) // 2 + (j - i)


_IU = [(i, j) for i in range(6) for j in range(i, 6)]


def _butterfly(x):
    for idx in _XOR:
        x = x + x[idx]
    return x[0]


def solve(H21, g, lam):
    """(H + lam diag(H_ii + 1e-9)) delta = -g by Cholesky, the operations in the header's order; None for a pivot that is not positive."""
    H21 = [float(v) for v in H21]
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        s = H21[hidx(j, j)] + lam * (H21[hidx(j, j)] + 1e-9)
        for k in range(j):
            s -= L[j][k] * L[j][k]
        if not s > 0.0:
            return None
        L[j][j] = float(np.sqrt(s))
        for i in range(j + 1, 6):
            v = H21[hidx(j, i)]
            for k in range(j):
                v -= L[i][k] * L[j][k]
            L[i][j] = v / L[j][j]
    y = [0.0] * 6
    for i in range(6):
        v = -float(g[i])
        for k in range(i):
            v -= L[i][k] * y[k]
        y[i] = v / L[i][i]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        v = y[i]
        for k in range(i + 1, 6):
            v -= L[k][i] * x[k]
        x[i] = v / L[i][i]
    x = np.array(x)
    return x if np.isfinite(x).all() else None


def rodrigues(w):
    th2 = float((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    th = float(np.sqrt(th2))
    sa, sb = 1.0, 0.5
    if th > 0.0:
        sh = float(np.sin(0.5 * th))
        sa = float(np.sin(th)) / th
        sb = ((2.0 * sh) * sh) / (th * th)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    K2 = np.outer(w, w) - th2 * np.eye(3)
    return np.eye(3) + (sa * K + sb * K2)


def _mat3(A, B):
    return np.array([[(A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j] for j in range(3)] for i in range(3)])


def lm_loop(evaluate, value, better, gain, follow, cur, R, t, ftol, max_iter, jitter=None, trace=None):
    """The iteration from `cur`, the caller's evaluation at (R, t), when there is anything to `follow`. `evaluate(R, t)` gives a dict with
    c, H and g, `value(ev)` the number that is followed, `better(trial, cur)` whether a trial is accepted, `gain(before, after)` what an
    accepted step won. `jitter`, a seeded generator, multiplies each component of every delta by 1 +- 2^-52; `trace`, a list, receives the
    value at the start and after every accepted step. Returns a dict of the last accepted evaluation and motion (`cur`, `R`, `t`), its
    `value`, `lam`, `iterations`, `accepted`, `reason` and `decision_margin`."""
    E = value(cur)
    if trace is not None:
        trace.append(E)
    lam, iterations, accepted, reason, margin = 1e-3, 0, 0, 2, np.inf
    if not follow:
        reason = 0
    else:
        while iterations < max_iter:
            delta = solve(cur["H"], cur["g"], lam)
            if delta is None:
                iterations += 1
                lam *= 8.0
                margin = min(margin, abs(lam - 1e8) / 1e8)
                if lam > 1e8:
                    reason = 3
                    break
                continue
            if jitter is not None:
                delta = delta * (1.0 + jitter.choice([-1.0, 1.0], size=6) * 2.0**-52)
            Rd = rodrigues(delta[:3])
            Rt = _mat3(Rd, R)
            w = t - cur["c"]
            tt = np.array([(((Rd[i, 0] * w[0] + Rd[i, 1] * w[1]) + Rd[i, 2] * w[2]) + cur["c"][i]) + delta[3 + i] for i in range(3)])
            tr = evaluate(Rt, tt)
            iterations += 1
            Et = value(tr)
            if not (Et == 0.0 and E == 0.0):
                margin = min(margin, abs(Et - E) / E)
            if better(Et, E):
                before = E
                accepted += 1
                cur, R, t, E = tr, Rt, tt, Et
                if trace is not None:
                    trace.append(E)
                lam = max(lam / 4.0, 1e-9)
                margin = min(margin, abs(gain(before, Et) - ftol * before) / before)
                if gain(before, Et) <= ftol * before:
                    reason = 1
                    break
            else:
                lam *= 8.0
                margin = min(margin, abs(lam - 1e8) / 1e8)
                if lam > 1e8:
                    reason = 3
                    break
    return dict(cur=cur, R=R, t=t, value=E, lam=lam, iterations=iterations, accepted=accepted, reason=reason, decision_margin=margin)


def net_motion(R, R0, accepted, c, c_start):
    """(angle, shift): the net rotation angle from the start, atan2(|vee(Q - Q^T)| / 2, (tr Q - 1) / 2) of Q = R R0^T - 0 when no step was
    accepted - and how far the centroid went."""
    Q = np.array([[(R[i, 0] * R0[j, 0] + R[i, 1] * R0[j, 1]) + R[i, 2] * R0[j, 2] for j in range(3)] for i in range(3)])
    a0, a1, a2 = Q[2, 1] - Q[1, 2], Q[0, 2] - Q[2, 0], Q[1, 0] - Q[0, 1]
    sn, cs = 0.5 * np.sqrt((a0 * a0 + a1 * a1) + a2 * a2), 0.5 * (((Q[0, 0] + Q[1, 1]) + Q[2, 2]) - 1.0)
    angle = float(np.arctan2(sn, cs)) if accepted else 0.0
    h = c - c_start
    return angle, float(np.sqrt((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]))
