"""A NumPy restatement of what `pmx_align` answers, for the align tests, on top of tests/explain_ref.py's `Tables` (`_matches`, `pos`): the
pair list of a (record, conformer, key), the weighted rigid fit by SVD (Kabsch with the determinant correction - on purpose not the
kernel's quaternion method; `method="horn"` is that one, through `numpy.linalg.eigh`), the residuals and the eigenvalue gap of Horn's
matrix. float64 throughout."""

from __future__ import annotations

import numpy as np

from explain_ref import NONE, Tables, candidates


def node_centers(model) -> np.ndarray:
    return np.array([model.nodes[m].center for m in range(model.num_nodes)], dtype=np.float64).reshape(-1, 3)


def pair_list(model, T: Tables, levels, key, c: int):
    """[(u, x_u, [m], [w])]: per fitted node, in record order, its position in conformer c and its partners in model-node order. Pairs
    whose weight is not > 0 are left out; a node that keeps no pair is not fitted."""
    out = []
    for l, lc in enumerate(levels):
        if int(key[l]) == NONE:
            continue
        for u, ms, w in T._matches(int(lc), int(key[l])):
            keep = [(m, float(x)) for m, x in zip(ms, w) if x > 0]
            if keep:
                out.append((u, T.pos[u, c].astype(np.float64), [m for m, _ in keep], np.array([x for _, x in keep])))
    return out


def horn_matrix(S: np.ndarray) -> np.ndarray:
    (sxx, sxy, sxz), (syx, syy, syz), (szx, szy, szz) = S
    return np.array([
        [sxx + syy + szz, syz - szy, szx - sxz, sxy - syx],
        [syz - szy, sxx - syy - szz, sxy + syx, szx + sxz],
        [szx - sxz, sxy + syx, -sxx + syy - szz, syz + szy],
        [sxy - syx, szx + sxz, syz + szy, -sxx - syy + szz],
    ])


def rotation_svd(S: np.ndarray) -> np.ndarray:
    U, _, Vt = np.linalg.svd(S)
    d = np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0
    return Vt.T @ np.diag([1.0, 1.0, d]) @ U.T


def rotation_horn(S: np.ndarray) -> np.ndarray:
    lam, vec = np.linalg.eigh(horn_matrix(S))
    q0, q1, q2, q3 = vec[:, int(np.argmax(lam))]
    return np.array([
        [q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
        [2 * (q1 * q2 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * (q2 * q3 - q0 * q1)],
        [2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3],
    ])


def align(model, rec, weights7, levels, key, c: int, tables: Tables | None = None, method: str = "svd", centers: np.ndarray | None = None) -> dict:
    """The fit of the match `key` (model cluster or -1 per level) for conformer c. valid: c is a conformer and every match a candidate of
    its level. R, t, W, sse, rmsd, rn (= rmsd_nodes^2 W), rmsd_nodes, E0, gap, spread (= sum_u sum_m w |y_m - ybar_u|^2), node [n] (-1
    for a node without a pair), n_nodes, n_pairs, and per fitted node u `posed[u]` and `target[u]` (its targets' weighted centroid)."""
    T = tables or Tables(model, rec, weights7)
    Y = node_centers(model) if centers is None else centers
    nl, n = len(levels), int(rec["n_nodes"])
    key = [int(k) for k in key] + [NONE] * (nl - len(key))
    valid = 0 <= c < T.C and all(k == NONE for k in key[nl:])
    valid = valid and all(key[l] == NONE or key[l] in candidates(model, rec, int(levels[l])) for l in range(nl))
    if not valid:
        return dict(valid=False)
    pl = pair_list(model, T, levels, key[:nl], c)
    out = dict(valid=True, R=np.eye(3), t=np.zeros(3), W=0.0, sse=0.0, rmsd=0.0, rn=0.0, rmsd_nodes=0.0, E0=0.0, gap=0.0, spread=0.0,
               node=np.full(n, -1.0), n_nodes=len(pl), n_pairs=sum(len(ms) for _, _, ms, _ in pl), posed={}, target={})
    if not pl:
        return out
    x = np.array([xu for _, xu, ms, _ in pl for _ in ms])
    y = np.array([Y[m] for _, _, ms, _ in pl for m in ms])
    w = np.concatenate([wu for _, _, _, wu in pl])
    W = float(w.sum())
    xb, yb = (w[:, None] * x).sum(0) / W, (w[:, None] * y).sum(0) / W
    S = (w[:, None] * (x - xb)).T @ (y - yb)
    if len(pl) < 2:
        S = np.zeros((3, 3))  # (pmx_align: one fitted node is its own centroid; R = I)
    R = np.eye(3) if len(pl) < 2 else (rotation_svd(S) if method == "svd" else rotation_horn(S))
    t = yb - R @ xb
    lam = np.linalg.eigvalsh(horn_matrix(S))
    sse = float((w * (((x @ R.T + t) - y) ** 2).sum(1)).sum())
    rn = spread = 0.0
    for u, xu, ms, wu in pl:
        yu = (wu[:, None] * Y[ms]).sum(0) / wu.sum()
        p = R @ xu + t
        out["posed"][u], out["target"][u] = p, yu
        out["node"][u] = float(np.linalg.norm(p - yu))
        rn += float(wu.sum() * ((p - yu) ** 2).sum())
        spread += float((wu * ((Y[ms] - yu) ** 2).sum(1)).sum())
    out.update(R=R, t=t, W=W, sse=sse, rmsd=float(np.sqrt(sse / W)), rn=rn, rmsd_nodes=float(np.sqrt(rn / W)),
               E0=float((w * (((x - xb) ** 2).sum(1) + ((y - yb) ** 2).sum(1))).sum()), gap=float(lam[-1] - lam[-2]), spread=spread)
    return out
