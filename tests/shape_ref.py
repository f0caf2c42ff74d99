"""NumPy restatement of `pmx_pose_shape` (include/pmx.h): the first-order Gaussian shape overlap of a posed row with a reference ligand.

Every term is formed by the header's operations in float64 - elementwise NumPy, which neither fuses nor reorders - and every sum is a
scalar loop in the specified order: a point's terms in ascending atom, a lane's points (point % 64) in ascending order, the 64 lanes by the
fixed butterfly. Everything but `np.exp` is correctly rounded, so the device differs from this file through `exp` alone; the integer outputs
depend on no `exp` at all. `margin` says how close a row stands to a place where an integer could still differ."""

import numpy as np

KAPPA = 2.4179879310247046
PI = 3.141592653589793
MAX_ATOMS = 256
OK, UNSUPPORTED, KEY_INVALID = 0, 1, 4


def alpha(radius):
    r = np.asarray(radius, dtype=np.float32).astype(np.float64)
    return KAPPA / (r * r)


def pose(points, R, t):
    """The posed point of include/pmx.h: p_k = ((R[k][0] x_0 + R[k][1] x_1) + R[k][2] x_2) + t_k."""
    x = np.asarray(points, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    R, t = np.asarray(R, dtype=np.float64).reshape(3, 3), np.asarray(t, dtype=np.float64).reshape(3)
    return np.stack([((R[k, 0] * x[:, 0] + R[k, 1] * x[:, 1]) + R[k, 2] * x[:, 2]) + t[k] for k in range(3)], axis=1).reshape(-1, 3)


def dist2(p, y):
    """d2 of point p [3] to every row of y [k, 3]: e = p - y, (e0 e0 + e1 e1) + e2 e2."""
    e = p[None, :] - y
    return (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]


def pair_terms(d2, alpha_a, alpha_b):
    s = alpha_a + alpha_b
    q = PI / s
    k = (alpha_a * alpha_b) / s
    return (8.0 * (q * np.sqrt(q))) * np.exp(-(k * d2))


def ordered_sum(values) -> float:
    acc = 0.0
    for v in values:
        acc = acc + float(v)
    return acc


def lane_sum(values) -> float:
    """A lane's entries (index % 64) in ascending order, then the butterfly: at step k lanes i and i ^ k both form v_i + v_(i ^ k)."""
    values = np.asarray(values, dtype=np.float64)
    lanes = np.array([ordered_sum(values[lane::64]) for lane in range(64)], dtype=np.float64)
    idx = np.arange(64)
    k = 1
    while k < 64:
        lanes = lanes + lanes[idx ^ k]
        k <<= 1
    return float(lanes[0])


def _first_min(d2):
    """(the smallest value, the lowest index that attains it, the gap to the next distinct value)."""
    j = int(np.argmin(d2))  # (the first among equals)
    rest = d2[d2 > d2[j]]
    return float(d2[j]), j, (float(rest.min() - d2[j]) if len(rest) else np.inf)


def self_overlap(ref_xyz, ref_radius) -> float:
    """O_BB: the O_AA of the reference's own atoms as a row under the identity motion."""
    return shape_row(ref_xyz, ref_radius, ref_xyz, ref_radius, np.eye(3), np.zeros(3), o_bb=0.0)["sums"][1]


def shape_row(ref_xyz, ref_radius, points, radii, R, t, cover=2.0, status=OK, o_bb=None):
    """One row. `radii`: per point, or one float32 for all. `status`: what the row front end says of a node-mode row before anything is
    read (an index outside the library, a conformer that is none); a motion that is not finite, a bad radius and a row of more than 256
    points are found here. Returns summary [10], counts [4], point_near, point_ref, ref_near [m], ref_point [m], status, sums (O_AB, O_AA,
    S_A, S_B, S_O) and margin."""
    y = np.asarray(ref_xyz, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    ab = alpha(ref_radius)
    m = len(y)
    x = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    npts = len(x)
    rad = np.broadcast_to(np.asarray(radii, dtype=np.float32), (npts,)) if np.ndim(radii) == 0 else np.asarray(radii, dtype=np.float32).reshape(-1)
    assert len(rad) == npts
    if o_bb is None:
        o_bb = self_overlap(ref_xyz, ref_radius)
    if status == OK and not (np.isfinite(np.asarray(R, dtype=np.float64)).all() and np.isfinite(np.asarray(t, dtype=np.float64)).all()):
        status = KEY_INVALID
    if status == OK and npts > MAX_ATOMS:
        status = UNSUPPORTED
    if status == OK and npts and not (np.isfinite(rad) & (rad > 0)).all():
        status = KEY_INVALID
    if status != OK:
        return dict(summary=np.full(10, np.nan), counts=np.zeros(4, np.int64), point_near=np.full(npts, np.nan), point_ref=np.full(npts, -1, np.int64),
                    ref_near=np.full(m, np.nan), ref_point=np.full(m, -1, np.int64), status=status, sums=(np.nan,) * 5, margin=np.inf)
    c2 = float(np.float64(np.float32(cover)) * np.float64(np.float32(cover)))
    p, aa = pose(x, R, t), alpha(rad)
    margin = np.inf
    cross, selfs, near2, point_ref = np.zeros(npts), np.zeros(npts), np.zeros(npts), np.zeros(npts, np.int64)
    for a in range(npts):
        d2 = dist2(p[a], y)
        cross[a] = ordered_sum(pair_terms(d2, aa[a], ab))
        selfs[a] = ordered_sum(pair_terms(dist2(p[a], p), aa[a], aa))
        near2[a], point_ref[a], gap = _first_min(d2)
        margin = min(margin, gap, abs(near2[a] - c2))
    ref_near2, ref_point = np.full(m, np.inf), np.full(m, -1, np.int64)
    if npts:
        for b in range(m):
            e = p - y[b][None, :]  # (p - y, as on the other side: the same bits)
            d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
            ref_near2[b], ref_point[b], gap = _first_min(d2)
            margin = min(margin, gap, abs(ref_near2[b] - c2))
    o_ab, o_aa, s_a, s_b = lane_sum(cross), lane_sum(selfs), lane_sum(near2), lane_sum(ref_near2)
    s_o = np.nan
    if npts == m:
        e = p - y
        s_o = lane_sum((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    summary = ratios(o_ab, o_aa, o_bb, s_a, s_b, s_o, npts, m)
    counts = np.array([npts, int((near2 < c2).sum()), int((ref_near2 < c2).sum()), m], dtype=np.int64)
    return dict(summary=summary, counts=counts, point_near=np.sqrt(near2), point_ref=point_ref, ref_near=np.sqrt(ref_near2), ref_point=ref_point, status=OK,
                sums=(o_ab, o_aa, s_a, s_b, s_o), margin=margin)


def ratios(o_ab, o_aa, o_bb, s_a, s_b, s_o, npts, m):
    """summary [10] from the row's sums, by the header's formulas (division and square root are correctly rounded on both sides)."""
    with np.errstate(all="ignore"):
        f = np.float64
        o_ab, o_aa, o_bb, s_a, s_b, s_o = f(o_ab), f(o_aa), f(o_bb), f(s_a), f(s_b), f(s_o)
        return np.array([o_ab, o_aa, o_bb, o_ab / ((o_aa + o_bb) - o_ab), o_ab / o_bb, f(0.0) if o_aa == 0.0 else o_ab / o_aa,
                         np.sqrt(s_a / f(npts)) if npts else np.nan, np.sqrt(s_b / f(m)), np.sqrt(s_o / f(m)) if npts == m else np.nan, 0.0], dtype=np.float64)


def random_rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(n, 3, 3)


POINT_COUNTS = (0, 1, 63, 64, 65, 128, 255, 256)  # where the trips of a lane per point change
REF_SIZES = (1, 63, 64, 65, 256)  # ... and those of a lane per reference atom
EXTRA_COUNTS = (3, 17, 41, 100, 200)
NODE_RADIUS, COVER = np.float32(1.25), 2.0
_cases = {}


def gpu_case(m, with_radii=True):
    """The seeded case the GPU tests run at reference size m, with the restatement of every row: computed once. Its seeds are the ones
    tests/test_shape_cpu.py finds every margin >= 1e-9 for."""
    key = (m, with_radii)
    if key not in _cases:
        counts = POINT_COUNTS + EXTRA_COUNTS
        ref_xyz, ref_radius, points, radii, R, t = seeded_case(9000 + m + (0 if with_radii else 500), m, counts, with_radii)
        o_bb = self_overlap(ref_xyz, ref_radius)
        rows = [shape_row(ref_xyz, ref_radius, points[i], radii[i] if with_radii else NODE_RADIUS, R[i], t[i], COVER, o_bb=o_bb) for i in range(len(counts))]
        _cases[key] = (ref_xyz, ref_radius, points, radii, R, t, rows)
    return _cases[key]


ELEMENT_RADII = np.array([1.47, 1.52, 1.55, 1.6, 1.7, 1.8, 1.98], np.float32)


def seeded_case(seed, m, counts, with_radii=True):
    """A reference of m atoms in a box of 8 A and one row per entry of `counts`: that many random points of a box of 10 A under a random
    proper rotation and a shift of up to 1 A. Returns (ref_xyz, ref_radius, points, radii or None, R, t)."""
    rng = np.random.default_rng(seed)
    ref_xyz = rng.uniform(-4, 4, size=(m, 3)).astype(np.float32)
    ref_radius = rng.choice(ELEMENT_RADII, size=m)
    points = [rng.uniform(-5, 5, size=(int(c), 3)).astype(np.float32) for c in counts]
    radii = [rng.choice(ELEMENT_RADII, size=int(c)) for c in counts] if with_radii else None
    return ref_xyz, ref_radius, points, radii, random_rotations(rng, len(counts)), rng.uniform(-1, 1, size=(len(counts), 3))
