"""The seeded rows of the refinement tests: tests/test_gpu_refine.py runs them on the GPU, tests/test_refine_cpu.py measures over exactly
these rows how far rounding moves the restatement (the sensitivity figure S) and checks that no row stands near a decision. A case is 64
rows of random points under random proper rotations inside a random shell pocket with a cavity, so that rows clash partly, not hopelessly.

ftol. A row that stops by reason 1 has taken a step with 0 < decrease <= ftol E, which lies within ftol of the threshold: with the default
ftol = 1e-9 no such row could have a decision margin of 1e-9. The cases therefore run at ftol = 1e-6, where a converging row's decreases fall
through the threshold in steps of a factor of ten and more."""

from functools import lru_cache

import numpy as np

import refine_ref

ROWS = 64
COUNTS = (0, 1, 2, 63, 64, 65, 130)
POCKET_SIZES = (0, 1, 64, 65, 497)
ANCHOR_COUNTS = (0, 1, 64, 65, 130)
MAX_ITERS = (0, 1, 32)
FTOL = 1e-6
RESTRAINT = 0.1
NODE_RADIUS = 1.25
TOLERANCE = 0.5
MARGIN = 1e-9

# name -> (pocket atoms, radii per point, anchors: None (own points) or (targets, weights), max_iter, seed)
CASES = {
    "points": (497, False, None, 32, 0),
    "radii": (497, True, None, 32, 0),
    "pocket0": (0, False, None, 32, 0),
    "pocket1": (1, False, None, 32, 22),
    "pocket64": (64, True, None, 32, 1),
    "pocket65": (65, False, None, 32, 0),
    "anchors": (497, False, (False, False), 32, 5),
    "anchors_t": (497, True, (True, False), 32, 10),
    "anchors_w": (497, False, (False, True), 32, 15),
    "anchors_tw": (497, True, (True, True), 32, 2),
    "iter0": (497, False, None, 0, 0),
    "iter1": (497, True, (True, True), 1, 0),
}


def random_rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(n, 3, 3)
    assert np.allclose(np.linalg.det(R), 1.0)
    return R


def ball(rng, n, radius):
    v = rng.normal(size=(n, 3))
    v /= np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12)
    return v * (radius * rng.random(n) ** (1.0 / 3.0))[:, None]


def shell_pocket(n_atoms, seed, inner=6.0, outer=10.0):
    """(xyz float32 [n, 3], radius float32 [n], group uint16 [n]): atoms between two spheres around the origin - a cavity of radius `inner`."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n_atoms, 3))
    v /= np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12)
    r = (inner**3 + (outer**3 - inner**3) * rng.random(n_atoms)) ** (1.0 / 3.0)
    xyz = (v * r[:, None]).astype(np.float32)
    radius = rng.choice(np.array([1.47, 1.52, 1.55, 1.6, 1.7, 1.8, 1.98], np.float32), size=n_atoms)
    group = rng.integers(0, 256, size=n_atoms).astype(np.uint16)
    return xyz, radius, group


@lru_cache(maxsize=None)
def case(name):
    """The inputs of a case: a dict of the pocket's arrays, and per row points, radii, anchors, targets, weights, R, t."""
    n_atoms, with_radii, anchors, max_iter, seed = CASES[name]
    rng = np.random.default_rng([n_atoms, int(with_radii), 0 if anchors is None else 1 + 2 * int(anchors[0]) + int(anchors[1]), max_iter, seed])
    n = ROWS
    counts = rng.choice(COUNTS, size=n)
    counts[: len(COUNTS)] = COUNTS  # (every count at least once)
    if anchors is not None:
        acounts = rng.choice(ANCHOR_COUNTS, size=n)
        acounts[: len(COUNTS) + 1] = (130, 65, 64, 130, 65, 64, 1, 0)  # (every count at least once, and not the point count of the same row)
        # A row held by one anchor or none can turn out of its clashes at no cost: its minimum is E = 0, which the iteration approaches
        # until E is rounding noise, and what it decides there is noise too. Such a row gets 130 points: too many to turn out of the shell.
        counts[acounts <= 1] = 130
    # points of the conformer's frame in a ball; the motion turns them and puts them off the cavity's centre, so that some reach the shell.
    # With few atoms the shell is narrower and the ball reaches through it: a pocket of one atom is still met
    reach = 4.5 if n_atoms >= 497 else 6.5
    points = [ball(rng, int(m), reach).astype(np.float32) for m in counts]
    radii = [rng.uniform(1.0, 2.0, size=int(m)).astype(np.float32) for m in counts] if with_radii else None
    R = random_rotations(rng, n)
    t = ball(rng, n, 1.5)
    anc = tgt = wts = None
    if anchors is not None:
        anc = [ball(rng, int(m), 4.0).astype(np.float32) for m in acounts]
        if anchors[0]:  # targets of their own: near where the start motion puts the anchors, not on it
            tgt = [a.astype(np.float64) @ R[i].T + t[i] + rng.normal(scale=0.3, size=(len(a), 3)) for i, a in enumerate(anc)]
        if anchors[1]:
            wts = [rng.uniform(0.0, 2.0, size=len(a)) for a in anc]
            for w in wts[::7]:
                w[: len(w) // 2] = 0.0  # (weights of exactly zero among them)
    xyz, radius, group = shell_pocket(n_atoms, 77 + n_atoms) if n_atoms >= 497 else shell_pocket(n_atoms, 77 + n_atoms, inner=3.0, outer=6.0)
    return dict(name=name, atom_xyz=xyz, atom_radius=radius, atom_group=group, points=points, radii=radii, anchors=anc, targets=tgt, weights=wts, R=R, t=t,
                max_iter=max_iter, n=n)


def reference_row(c, i, variant="forward", seed=0, **kw):
    pick = lambda v: None if v is None else v[i]  # noqa: E731
    args = dict(tolerance=TOLERANCE, restraint=RESTRAINT, ftol=FTOL, max_iter=c["max_iter"])
    args.update(kw)
    return refine_ref.refine_row(c["atom_xyz"], c["atom_radius"], c["points"][i], c["radii"][i] if c["radii"] is not None else np.float32(NODE_RADIUS), c["R"][i], c["t"][i],
                                 anchors=pick(c["anchors"]), targets=pick(c["targets"]), weights=pick(c["weights"]), variant=variant, seed=seed, **args)


@lru_cache(maxsize=None)
def reference(name, variant="forward"):
    """The restatement of every row of a case: computed once, shared by the tests, left unchanged."""
    c = case(name)
    return [reference_row(c, i, variant, seed=1000 + i) for i in range(c["n"])]


def sensitivity(name):
    """Over the rows of a case: (S_points, S_energy, agree, margin) - the largest difference between the three variants in posed point
    coordinates (A) and in relative final E, whether all three agree in status, iterations, accepted, stop and n_pairs on every row, and the
    smallest decision margin of any variant."""
    import clash_ref

    c = case(name)
    refs = [reference(name, v) for v in ("forward", "reverse", "jitter")]
    s_pts = s_e = 0.0
    agree, margin = True, np.inf
    for i in range(c["n"]):
        rows = [r[i] for r in refs]
        margin = min([margin] + [r["decision_margin"] for r in rows])
        agree = agree and all(r["status"] == rows[0]["status"] and np.array_equal(r["count"], rows[0]["count"]) for r in rows[1:])
        if rows[0]["status"] != 0:
            continue
        posed = [clash_ref.pose(c["points"][i], r["rotation"], r["translation"]) for r in rows]
        E = [r["energy"][2] + RESTRAINT * r["energy"][3] for r in rows]
        for k in (1, 2):
            if len(posed[0]):
                s_pts = max(s_pts, float(np.abs(posed[k] - posed[0]).max()))
            if E[0] > 0:
                s_e = max(s_e, abs(E[k] - E[0]) / E[0])
    return s_pts, s_e, agree, margin

# The sensitivity figure of each case as tests/test_refine_cpu.py measures it (the larger of the difference in posed points, in A, and in
# relative final E between the three variants of the restatement), recorded as measured and not rounded. The largest are the thin pockets'
# rows that run out of iterations far from a minimum. A case's bar on the GPU is max(1e-12, 1000 S[case]).
S = {
    "points": 7.216134297708249e-15,
    "radii": 3.419486915845482e-14,
    "pocket0": 0.0,
    "pocket1": 2.6645352591003757e-15,
    "pocket64": 2.19966267422933e-11,
    "pocket65": 7.02016222930979e-12,
    "anchors": 2.589040093425865e-13,
    "anchors_t": 1.0436096431476471e-14,
    "anchors_w": 3.175237850427948e-14,
    "anchors_tw": 2.4646951146678475e-14,
    "iter0": 6.562722019788632e-16,
    "iter1": 1.7763568394002505e-15,
}


def bar(name):
    return max(1e-12, 1000 * S[name])
