"""The seeded rows of the colour tests: tests/test_gpu_pose_colour.py and tests/test_gpu_combo_overlay.py run them on the GPU,
tests/test_colour_cpu.py measures over exactly these rows how far rounding moves the restatement (the sensitivity figure S) and checks that
no row stands near a decision. A case is 64 rows against one known ligand - its atoms (the shape reference) and its typed features (the
colour reference, placed on atoms of it). Even rows are perturbed copies of it: atoms and features drawn with repetition, 0.3 A of noise
each, turned by 0.2 to 0.5 rad about the ligand's centre and shifted by 1 to 2 A. Odd rows are random typed molecules: a ball of points
and a ball of typed nodes under a random proper rotation, the centre within 1.5 A of the ligand's. So a row neither sits at a maximum nor
has F = 0, but for the rows without any point.

A row is a record of a library on the GPU (`library`): its typed nodes at conformer 1 of 2 - conformer 0 holds other coordinates - so the
calls read a record with a stride. Its shape points are a point set of their own (the cases with `points`), or the nodes themselves.

ftol is 1e-6, as in tests/overlay_cases.py and for the reason given there."""

import struct
from functools import lru_cache

import numpy as np

import colour_ref
import combo_ref
import shape_ref
from overlay_cases import ball, reference_atoms, rotation_about

ROWS = 64
NODE_COUNTS = (0, 1, 2, 63, 64)
EXTRA_NODE_COUNTS = (7, 20, 33)
POINT_COUNTS = (0, 1, 63, 64, 65, 255, 256)
EXTRA_POINT_COUNTS = (10, 30, 128)
FEATURE_SIZES = (1, 2, 63, 64)
MAX_ITERS = (0, 1, 32)
FTOL = 1e-6
NODE_RADIUS = 1.25
COLOUR_RADIUS = 1.0
COVER = 2.0
MARGIN = 1e-9
BIG_ROWS = 3  # rows of 256 points against the reference of 256 atoms
DEFAULT = (1.0, 4.0, 8.0, 8.0, 4.0, 4.0, 4.0)  # constants.DEFAULT_WEIGHTS in TYPE_NAMES order
NO_HYDROPHOBIC = (0.0, 4.0, 8.0, 8.0, 4.0, 4.0, 4.0)  # a set with a zero weight

# name -> (reference atoms m, features f, a point set per row, weights, colour_weight (None: balanced), max_iter)
CASES = {
    "f1": (41, 1, True, DEFAULT, 1.0, 32),
    "f2_nodes": (2, 2, False, NO_HYDROPHOBIC, None, 32),
    "f63": (65, 63, True, DEFAULT, None, 32),
    "f64": (64, 64, True, NO_HYDROPHOBIC, 1.0, 32),
    "cw0": (41, 20, True, DEFAULT, 0.0, 32),
    "big": (256, 64, True, DEFAULT, None, 32),
    "iter0": (41, 20, True, DEFAULT, 1.0, 0),
    "iter1": (65, 20, False, NO_HYDROPHOBIC, None, 1),
}
# (chosen so that every row of every variant stands at least 1e-8 off every decision: tests/test_colour_cpu.py asserts 1e-9)
SEEDS = {"f1": 11, "f2_nodes": 8, "f63": 7, "f64": 8, "cw0": 1, "big": 11, "iter0": 0, "iter1": 0}


def random_masks(rng, n, zero=True):
    """Type masks: six in ten of one type, three in ten of two or three, one in ten 0 (`zero`)."""
    kind = rng.choice(3, size=n, p=[0.6, 0.3, 0.1] if zero else [0.65, 0.35, 0.0])
    out = np.zeros(n, np.uint8)
    for i in range(n):
        if kind[i] == 0:
            out[i] = 1 << int(rng.integers(0, 7))
        elif kind[i] == 1:
            out[i] = sum(1 << int(t) for t in rng.choice(7, size=int(rng.integers(2, 4)), replace=False))
    return out


@lru_cache(maxsize=None)
def case(name):
    """The inputs of a case: the two references, and per row nodes, masks, points (None: the nodes), radii, R, t."""
    m, f, with_points, weights, cw, max_iter = CASES[name]
    rng = np.random.default_rng([m, f, int(with_points), max_iter, SEEDS[name]])
    ref_xyz, ref_radius = reference_atoms(m, rng)
    feat_xyz = ref_xyz[rng.integers(0, m, size=f)].copy()  # (features sit on atoms; with more features than atoms some coincide)
    feat_mask = random_masks(rng, f)
    if not feat_mask.any():
        feat_mask[0] = 1 << 3
    if f >= 20:
        feat_mask[:8] = [1, 2, 4, 8, 16, 32, 64, 0]  # every type, and a feature that pairs with nothing
    n = ROWS
    # Every count at least once. A row of fewer than two shape points has its centroid at the origin or on the one point, and the few typed
    # pairs that are left are followed to within rounding of their maximum, where the last decisions are noise (tests/overlay_cases.py has
    # the same to say of one point against one atom): such counts stand once each, next to a full set of the other kind.
    node_counts = rng.choice([c for c in NODE_COUNTS + EXTRA_NODE_COUNTS if c > 2], size=n)
    node_counts[: len(NODE_COUNTS)] = NODE_COUNTS
    usual = [c for c in POINT_COUNTS + EXTRA_POINT_COUNTS if 1 < c < (255 if m == 256 else 257)]
    point_counts = rng.choice(usual, size=n)
    point_counts[8: 8 + len(POINT_COUNTS)] = POINT_COUNTS
    if m == 256:
        point_counts[16: 16 + BIG_ROWS - 1] = 256  # (256 x 256 in a few rows only: BIG_ROWS with the one above)
    y = ref_xyz.astype(np.float64)
    cen = y.mean(axis=0)
    extent = max(float(np.linalg.norm(y - cen, axis=1).max()), 1.5)
    nodes, masks, points, radii, R, t = [], [], [], [], np.zeros((n, 3, 3)), np.zeros((n, 3))
    for i in range(n):
        nn, c = int(node_counts[i]), int(point_counts[i])
        axis, angle = rng.normal(size=3), rng.uniform(0.2, 0.5)
        shift = ball(rng, 1, 1.0)[0]
        shift = shift / max(np.linalg.norm(shift), 1e-12) * rng.uniform(1.0, 2.0)
        if i % 2 == 0:  # a perturbed copy
            pick = rng.integers(0, f, size=nn)
            nodes.append((feat_xyz[pick].astype(np.float64) - cen + rng.normal(scale=0.3, size=(nn, 3))).astype(np.float32))
            masks.append(feat_mask[pick].copy())
            pick = rng.integers(0, m, size=c)
            points.append((y[pick] - cen + rng.normal(scale=0.3, size=(c, 3))).astype(np.float32))
            radii.append(ref_radius[pick].astype(np.float32))
            R[i], t[i] = rotation_about(axis, angle), cen + shift
        else:  # a random typed molecule
            nodes.append(ball(rng, nn, extent).astype(np.float32))
            masks.append(random_masks(rng, nn))
            points.append(ball(rng, c, extent * (max(c, 1) / m) ** (1.0 / 3.0) if c < m else extent).astype(np.float32))
            radii.append(rng.choice(shape_ref.ELEMENT_RADII, size=c))
            R[i], t[i] = shape_ref.random_rotations(rng, 1)[0], cen + 0.75 * shift
    out = dict(name=name, ref_xyz=ref_xyz, ref_radius=ref_radius, feat_xyz=feat_xyz, feat_mask=feat_mask, weights=np.asarray(weights, np.float32), nodes=nodes, masks=masks,
               points=points if with_points else None, radii=radii if with_points else None, R=R, t=t, max_iter=max_iter, n=n)
    out["o_bb"] = shape_ref.self_overlap(ref_xyz, ref_radius)
    out["c_bb"] = colour_ref.self_overlap(feat_xyz, feat_mask, weights, COLOUR_RADIUS)
    out["cw"] = float(out["o_bb"] / out["c_bb"]) if cw is None else float(cw)  # balanced: O_BB / C_BB of the restatement
    return out


def shape_points(c, i):
    """(points, radii) of row i: its point set, or its nodes as spheres of NODE_RADIUS."""
    if c["points"] is None:
        return c["nodes"][i], np.float32(NODE_RADIUS)
    return c["points"][i], c["radii"][i]


def record(nodes, masks, conformers=2, at=1):
    """A library record of typed nodes (pharmaconet_amd/library.py's layout): the nodes at conformer `at`, other coordinates elsewhere;
    one cluster of all nodes."""
    nodes = np.asarray(nodes, dtype=np.float32).reshape(-1, 3)
    n = len(nodes)
    ncl = 1 if n else 0
    xyz = np.zeros((n, 3, conformers), np.float32)
    for c in range(conformers):
        xyz[:, :, c] = nodes if c == at else nodes[::-1] * np.float32(0.5) + np.float32(3.0 + c)
    body = struct.pack("<HHHH", n, conformers, ncl, 0) + np.asarray(masks, dtype=np.uint8).tobytes() + bytes([n] * ncl)
    body += b"\0" * ((-len(body)) % 4) + xyz.tobytes()
    return body + b"\0" * ((-len(body)) % 16)


@lru_cache(maxsize=None)
def library(name):
    """The rows of a case as a `PackedLibrary`, one record a row, and the conformer each row is read at."""
    from pharmaconet_amd import PackedLibrary

    c = case(name)
    return PackedLibrary.from_records([record(c["nodes"][i], c["masks"][i]) for i in range(c["n"])]), np.ones(c["n"], np.int64)


def reference_row(c, i, variant="forward", seed=0, **kw):
    pts, rad = shape_points(c, i)
    args = dict(ftol=FTOL, max_iter=c["max_iter"])
    args.update(kw)
    return combo_ref.combo_row(c["ref_xyz"], c["ref_radius"], c["feat_xyz"], c["feat_mask"], c["weights"], COLOUR_RADIUS, pts, rad, c["nodes"][i], c["masks"][i], c["R"][i], c["t"][i],
                               c["cw"], variant=variant, seed=seed, o_bb=c["o_bb"], c_bb=c["c_bb"], **args)


@lru_cache(maxsize=None)
def reference(name, variant="forward"):
    """The restatement of every row of a case: computed once, shared by the tests, left unchanged."""
    c = case(name)
    return [reference_row(c, i, variant, seed=1000 + i) for i in range(c["n"])]


@lru_cache(maxsize=None)
def colour_reference(name):
    """`colour_ref.colour_row` of every row's nodes at the input motion: what `pmx_pose_colour` is compared with."""
    c = case(name)
    return [colour_ref.colour_row(c["feat_xyz"], c["feat_mask"], c["weights"], COLOUR_RADIUS, c["nodes"][i], c["masks"][i], c["R"][i], c["t"][i], COVER, c_bb=c["c_bb"])
            for i in range(c["n"])]


def sensitivity(name):
    """Over the rows of a case: (S_points, S_F, agree, margin) - the largest difference between the three variants in posed point
    coordinates (A; shape points and nodes) and in relative final F, whether all three agree in status and the six counts on every row,
    and the smallest decision margin of any variant."""
    c = case(name)
    refs = [reference(name, v) for v in ("forward", "reverse", "jitter")]
    s_pts = s_f = 0.0
    agree, margin = True, np.inf
    for i in range(c["n"]):
        rows = [r[i] for r in refs]
        margin = min([margin] + [r["decision_margin"] for r in rows])
        agree = agree and all(r["status"] == rows[0]["status"] and np.array_equal(r["count"], rows[0]["count"]) for r in rows[1:])
        if rows[0]["status"] != 0:
            continue
        both = np.concatenate([np.asarray(shape_points(c, i)[0], np.float32).reshape(-1, 3), c["nodes"][i].reshape(-1, 3)])
        posed = [shape_ref.pose(both, r["rotation"], r["translation"]) for r in rows]
        F = [r["F"][1] for r in rows]
        for k in (1, 2):
            if len(both):
                s_pts = max(s_pts, float(np.abs(posed[k] - posed[0]).max()))
            if F[0] > 0:
                s_f = max(s_f, abs(F[k] - F[0]) / F[0])
    return s_pts, s_f, agree, margin


# The sensitivity figure of each case as tests/test_colour_cpu.py measures it (the larger of the difference in posed points, in A, and in
# relative final F between the three variants of the restatement), recorded as measured and not rounded. A case's bar on the GPU is
# max(1e-12, 1000 S[case]).
S = {
    "f1": 2.7533531010703882e-14,
    "f2_nodes": 1.7763568394002505e-15,
    "f63": 5.1514348342607263e-14,
    "f64": 3.552713678800501e-14,
    "cw0": 5.906386491005833e-14,
    "big": 2.220446049250313e-14,
    "iter0": 8.687413410366067e-16,
    "iter1": 5.329070518200751e-15,
}


def bar(name):
    return max(1e-12, 1000 * S[name])
