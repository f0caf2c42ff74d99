"""NumPy restatement of `pmx_pose_colour` (include/pmx.h): the typed first-order Gaussian overlap of a posed row of typed points with a
known ligand's pharmacophore features.

Every term is formed by the header's operations in float64 - elementwise NumPy, which neither fuses nor reorders - and every sum is taken
one term after the other in the specified order (`np.cumsum` adds one term at a time): a point's terms in ascending feature, a lane's one
point, the 64 lanes by the fixed butterfly. A pair whose weight is 0 is left out by adding +0.0 in its place, which changes no bit of a sum
of terms that are >= 0. Everything but `np.exp` is correctly rounded, so the device differs from this file through `exp` alone; the integer
outputs depend on no `exp` at all. `margin` says how close a row stands to a place where an integer could still differ."""

import numpy as np

import shape_ref
from shape_ref import KAPPA, KEY_INVALID, OK, UNSUPPORTED, lane_sum, pair_terms, pose  # noqa: F401

MAX_POINTS = 64
NUM_TYPES = 7


def weights64(weights):
    w = np.asarray(weights, dtype=np.float32).astype(np.float64).reshape(NUM_TYPES)
    assert np.isfinite(w).all() and (w >= 0).all()
    return w


def weight_table(weights):
    """w of every set of shared bits, [128]: the weights of the set's types added in ascending type from 0.0."""
    w = weights64(weights)
    table = np.zeros(128)
    for bits in range(128):
        acc = 0.0
        for t in range(NUM_TYPES):
            if (bits >> t) & 1:
                acc = acc + float(w[t])
        table[bits] = acc
    return table


def alpha_c(radius):
    r = np.float64(np.float32(radius))
    return float(KAPPA / (r * r))


def running(terms):
    """terms [n, m] summed over axis 1 one after the other, from 0.0."""
    terms = np.asarray(terms, dtype=np.float64)
    return np.cumsum(np.concatenate([np.zeros((terms.shape[0], 1)), terms], axis=1), axis=1)[:, -1]


def _nearest(d2, allowed):
    """Per row of d2 [n, m] over the allowed columns: (smallest value or inf, lowest index that attains it or -1, gap to the next distinct one)."""
    n = d2.shape[0]
    near2, index, gap = np.full(n, np.inf), np.full(n, -1, np.int64), np.full(n, np.inf)
    for i in range(n):
        cols = np.flatnonzero(allowed[i])
        if len(cols):
            v = d2[i, cols]
            j = int(np.argmin(v))  # (the first among equals)
            near2[i], index[i] = v[j], cols[j]
            rest = v[v > v[j]]
            gap[i] = float(rest.min() - v[j]) if len(rest) else np.inf
    return near2, index, gap


def self_overlap(ref_xyz, ref_mask, weights, radius) -> float:
    """C_BB: the C_AA of the reference's own features as a row under the identity motion."""
    return colour_row(ref_xyz, ref_mask, weights, radius, ref_xyz, ref_mask, np.eye(3), np.zeros(3), c_bb=0.0)["sums"][1]


def tanimoto(cab, caa, cbb):
    with np.errstate(all="ignore"):
        f = np.float64
        return 0.0 if cab == 0.0 else float(f(cab) / ((f(caa) + f(cbb)) - f(cab)))


def ratios(cab, caa, cbb, s, matched):
    """summary [8] from the row's sums, by the header's formulas."""
    with np.errstate(all="ignore"):
        f = np.float64
        cab, caa, cbb, s = f(cab), f(caa), f(cbb), f(s)
        return np.array([cab, caa, cbb, tanimoto(cab, caa, cbb), f(0.0) if cbb == 0.0 else cab / cbb, f(0.0) if caa == 0.0 else cab / caa,
                         np.sqrt(s / f(matched)) if matched else np.nan, 0.0], dtype=np.float64)


def not_ok(status):
    nan64, neg = np.full(MAX_POINTS, np.nan), np.full(MAX_POINTS, -1, np.int64)
    return dict(summary=np.full(8, np.nan), type_overlap=np.full(NUM_TYPES, np.nan), counts=np.zeros(4, np.int64), node_colour=nan64, node_near=nan64.copy(), node_feature=neg,
                feat_near=nan64.copy(), feat_node=neg.copy(), fp=0, status=status, sums=(np.nan,) * 3, margin=np.inf)


def colour_row(ref_xyz, ref_mask, weights, radius, points, masks, R, t, cover=2.0, status=OK, c_bb=None):
    """One row. `status`: what the row front end says of a node-mode row before anything is read; a motion that is not finite, a row of more
    than 64 typed points and a mask >= 128 are found here. Returns summary [8], type_overlap [7], counts [4], the per-node and per-feature
    arrays [64], fp (word 0 of matched_fp), status, sums (C_AB, C_AA, S) and margin."""
    y = np.asarray(ref_xyz, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    mb = np.asarray(ref_mask, dtype=np.int64).reshape(-1)
    f = len(y)
    assert 1 <= f <= MAX_POINTS and len(mb) == f and (mb < 128).all() and (mb >= 0).all()
    x = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    ma = np.asarray(masks, dtype=np.int64).reshape(-1)
    n = len(x)
    assert len(ma) == n
    if status == OK and not (np.isfinite(np.asarray(R, dtype=np.float64)).all() and np.isfinite(np.asarray(t, dtype=np.float64)).all()):
        status = KEY_INVALID
    if status == OK and n > MAX_POINTS:
        status = UNSUPPORTED
    if status == OK and n and (ma >= 128).any():
        status = KEY_INVALID
    if status != OK:
        return not_ok(status)
    W, table, al = weights64(weights), weight_table(weights), alpha_c(radius)
    if c_bb is None:
        c_bb = self_overlap(ref_xyz, ref_mask, weights, radius)
    c2 = float(np.float64(np.float32(cover)) * np.float64(np.float32(cover)))
    p = pose(x, R, t)
    # ---- the points against the features
    shared = ma[:, None] & mb[None, :]
    w = table[shared]
    e = p[:, None, :] - y[None, :, :]
    d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    with np.errstate(under="ignore"):
        V = pair_terms(d2, al, al)
    paired = w != 0.0
    cross = running(np.where(paired, w * V, 0.0))
    parts = np.stack([running(np.where(paired & (((shared >> k) & 1) == 1), W[k] * V, 0.0)) for k in range(NUM_TYPES)], axis=1)
    near2, node_feature, gap = _nearest(d2, paired)
    # ---- the points against the row itself
    ws = table[ma[:, None] & ma[None, :]]
    es = p[:, None, :] - p[None, :, :]
    d2s = (es[..., 0] * es[..., 0] + es[..., 1] * es[..., 1]) + es[..., 2] * es[..., 2]
    with np.errstate(under="ignore"):
        selfs = running(np.where(ws != 0.0, ws * pair_terms(d2s, al, al), 0.0))
    # ---- the features against the points (d2 from e = p - y, as above: the same bits)
    feat_near2, feat_node, fgap = _nearest(d2.T, paired.T)
    matched = node_feature >= 0
    margin = float(min([np.inf] + list(gap[matched]) + list(np.abs(near2[matched] - c2)) + list(fgap[feat_node >= 0]) + list(np.abs(feat_near2[feat_node >= 0] - c2))))
    cab, caa, s = lane_sum(cross), lane_sum(selfs), lane_sum(np.where(matched, near2, 0.0))
    type_overlap = np.array([lane_sum(parts[:, k]) for k in range(NUM_TYPES)])
    covered_f = (feat_node >= 0) & (feat_near2 < c2)
    counts = np.array([n, int((matched & (near2 < c2)).sum()), int(covered_f.sum()), f], dtype=np.int64)

    def padded(values, fill, dtype=np.float64):
        out = np.full(MAX_POINTS, fill, dtype=dtype)
        out[: len(values)] = values
        return out

    with np.errstate(invalid="ignore"):
        node_near = np.where(matched, np.sqrt(np.where(matched, near2, 0.0)), np.nan)
        feat_near = np.where(feat_node >= 0, np.sqrt(np.where(feat_node >= 0, feat_near2, 0.0)), np.nan)
    return dict(summary=ratios(cab, caa, c_bb, s, int(matched.sum())), type_overlap=type_overlap, counts=counts, node_colour=padded(cross, np.nan),
                node_near=padded(node_near, np.nan), node_feature=padded(node_feature, -1, np.int64), feat_near=padded(feat_near, np.nan),
                feat_node=padded(feat_node, -1, np.int64), fp=int(sum(1 << int(b) for b in np.flatnonzero(covered_f))), status=OK, sums=(cab, caa, s), margin=margin)
