"""The seeded rows of the shape-overlay tests: tests/test_gpu_shape_overlay.py runs them on the GPU, tests/test_overlay_cpu.py measures over
exactly these rows how far rounding moves the restatement (the sensitivity figure S) and checks that no row stands near a decision. A case
is 64 rows against one reference: even rows are perturbed copies of it (its atoms drawn with repetition, 0.3 A of noise each, turned by 0.2
to 0.5 rad about their centre and shifted by 1 to 2 A), odd rows random molecules (a ball of the reference's density under a random proper
rotation, its centre within 1.5 A of the reference's). So a row neither sits at a maximum nor has O_AB = 0; the case "flat" holds a few of
each of those two kinds, of which only the status, stop reason 0 and the bits of the input are asserted (a row at a maximum decides by
rounding noise: its trials change O_AB in the last bit or not at all).

ftol. A row that stops by reason 1 has taken a step with 0 < increase <= ftol O_AB, which lies within ftol of the threshold: the cases run at
ftol = 1e-6, as tests/refine_cases.py does and for the reason it gives."""

from functools import lru_cache

import numpy as np

import overlay_ref
import shape_ref
from conftest import GOLDEN

ROWS = 64
COUNTS = (0, 1, 2, 3, 63, 64, 65, 128, 255, 256)
REF_SIZES = (1, 2, 41, 64, 65, 256)
MAX_ITERS = (0, 1, 32)
FTOL = 1e-6
NODE_RADIUS = 1.25
MARGIN = 1e-9
BIG_ROWS = 3  # rows of 256 points against the reference of 256 atoms

# name -> (reference atoms, radii per point, max_iter, seed)
CASES = {
    "ref1": (1, True, 32, 0),
    "ref2": (2, False, 32, 0),
    "ref41": (41, True, 32, 0),
    "ref41_nodes": (41, False, 32, 0),
    "ref64": (64, True, 32, 0),
    "ref65": (65, False, 32, 0),
    "ref256": (256, True, 32, 0),
    "iter0": (41, True, 0, 0),
    "iter1": (65, True, 1, 0),
}


def ligand_6oim():
    """(xyz float32 [41, 3], radius float32 [41]) of tests/golden/ligand_6oim_mov.pdb, as `ReferenceLigand.from_pdb` reads it."""
    from pharmaconet_amd.shape import ReferenceLigand

    ref = ReferenceLigand.from_pdb(GOLDEN / "ligand_6oim_mov.pdb")
    assert len(ref) == 41
    return ref.xyz, ref.radius


def ball(rng, n, radius):
    v = rng.normal(size=(n, 3))
    v /= np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12)
    return v * (radius * rng.random(n) ** (1.0 / 3.0))[:, None]


def rotation_about(axis, angle):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def reference_atoms(m, rng):
    """A reference of m atoms: the 6OIM ligand at 41, otherwise a chain-like random molecule (a walk of 1.5 A bonds kept 1.2 A apart where it
    can be)."""
    if m == 41:
        return ligand_6oim()
    xyz = np.zeros((m, 3))
    for i in range(1, m):
        for _ in range(20):
            step = rng.normal(size=3)
            cand = xyz[rng.integers(max(0, i - 3), i)] + 1.5 * step / np.linalg.norm(step)
            if np.linalg.norm(xyz[:i] - cand, axis=1).min() > 1.2:
                break
        xyz[i] = cand
    return (xyz + rng.uniform(-3, 3, size=3)).astype(np.float32), rng.choice(shape_ref.ELEMENT_RADII, size=m)


@lru_cache(maxsize=None)
def case(name):
    """The inputs of a case: the reference's arrays, and per row points, radii (or None), R, t."""
    m, with_radii, max_iter, seed = CASES[name]
    rng = np.random.default_rng([m, int(with_radii), max_iter, seed])
    ref_xyz, ref_radius = reference_atoms(m, rng)
    n = ROWS
    small = [c for c in COUNTS if c < 255]
    counts = rng.choice(small if m == 256 else COUNTS, size=n)
    counts[: len(COUNTS)] = COUNTS  # (every count at least once)
    if m == 1:
        # One point against one atom has its maximum where the two coincide, and the iteration lands on it within rounding in three steps
        # (the surrogate is exact there): such a row sits at a maximum, and its last decisions are noise. One point meets 2 to 256 atoms
        # in the other cases.
        counts[counts == 1] = 2
    if m == 256:
        counts[len(COUNTS): len(COUNTS) + BIG_ROWS - 1] = 256  # (256 x 256 in a few rows only: BIG_ROWS with the one above)
    y = ref_xyz.astype(np.float64)
    cen = y.mean(axis=0)
    extent = max(float(np.linalg.norm(y - cen, axis=1).max()), 1.5)
    points, radii, R, t = [], [], np.zeros((n, 3, 3)), np.zeros((n, 3))
    for i, c in enumerate(int(c) for c in counts):
        axis, angle = rng.normal(size=3), rng.uniform(0.2, 0.5)
        shift = ball(rng, 1, 1.0)[0]
        shift = shift / max(np.linalg.norm(shift), 1e-12) * rng.uniform(1.0, 2.0)
        if i % 2 == 0:  # a perturbed copy
            pick = rng.integers(0, m, size=c)
            points.append((y[pick] - cen + rng.normal(scale=0.3, size=(c, 3))).astype(np.float32))
            radii.append(ref_radius[pick].astype(np.float32))
            R[i], t[i] = rotation_about(axis, angle), cen + shift
        else:  # a random molecule
            points.append(ball(rng, c, extent * (max(c, 1) / m) ** (1.0 / 3.0) if c < m else extent).astype(np.float32))
            radii.append(rng.choice(shape_ref.ELEMENT_RADII, size=c))
            R[i], t[i] = shape_ref.random_rotations(rng, 1)[0], cen + 0.75 * shift
    return dict(name=name, ref_xyz=ref_xyz, ref_radius=ref_radius, points=points, radii=radii if with_radii else None, R=R, t=t, max_iter=max_iter, n=n)


@lru_cache(maxsize=None)
def flat_case():
    """Rows with nothing to follow, against the 6OIM ligand: its own atoms in place (a maximum, Tanimoto exactly 1), and rows 200 A and more
    away, where every term underflows (stop 0, the input's bits)."""
    ref_xyz, ref_radius = ligand_6oim()
    rng = np.random.default_rng(41)
    n_far = 4
    points = [ref_xyz.copy() for _ in range(3)] + [ball(rng, c, 4.0).astype(np.float32) for c in (1, 41, 64, 256)[:n_far]]
    radii = [ref_radius.copy() for _ in range(3)] + [rng.choice(shape_ref.ELEMENT_RADII, size=len(p)) for p in points[3:]]
    R = np.concatenate([np.eye(3)[None].repeat(3, axis=0), shape_ref.random_rotations(rng, n_far)])
    t = np.concatenate([np.zeros((3, 3)), ref_xyz.astype(np.float64).mean(axis=0) + 200.0 * np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1.5], [-1, -1, -1]])[:n_far]])
    return dict(name="flat", ref_xyz=ref_xyz, ref_radius=ref_radius, points=points, radii=radii, R=R, t=t, max_iter=32, n=len(points), at_maximum=np.arange(3), far=np.arange(3, 3 + n_far))


def reference_row(c, i, variant="forward", seed=0, **kw):
    args = dict(ftol=FTOL, max_iter=c["max_iter"])
    args.update(kw)
    return overlay_ref.overlay_row(c["ref_xyz"], c["ref_radius"], c["points"][i], c["radii"][i] if c["radii"] is not None else np.float32(NODE_RADIUS), c["R"][i], c["t"][i],
                                   variant=variant, seed=seed, o_bb=self_overlap(c["name"]), **args)


@lru_cache(maxsize=None)
def self_overlap(name):
    c = flat_case() if name == "flat" else case(name)
    return shape_ref.self_overlap(c["ref_xyz"], c["ref_radius"])


@lru_cache(maxsize=None)
def reference(name, variant="forward"):
    """The restatement of every row of a case: computed once, shared by the tests, left unchanged."""
    c = case(name)
    return [reference_row(c, i, variant, seed=1000 + i) for i in range(c["n"])]


def sensitivity(name):
    """Over the rows of a case: (S_points, S_overlap, agree, margin) - the largest difference between the three variants in posed point
    coordinates (A) and in relative final O_AB, whether all three agree in status and the four counts on every row, and the smallest
    decision margin of any variant."""
    c = case(name)
    refs = [reference(name, v) for v in ("forward", "reverse", "jitter")]
    s_pts = s_o = 0.0
    agree, margin = True, np.inf
    for i in range(c["n"]):
        rows = [r[i] for r in refs]
        margin = min([margin] + [r["decision_margin"] for r in rows])
        agree = agree and all(r["status"] == rows[0]["status"] and np.array_equal(r["count"], rows[0]["count"]) for r in rows[1:])
        if rows[0]["status"] != 0:
            continue
        posed = [shape_ref.pose(c["points"][i], r["rotation"], r["translation"]) for r in rows]
        O = [r["energy"][1] for r in rows]
        for k in (1, 2):
            if len(posed[0]):
                s_pts = max(s_pts, float(np.abs(posed[k] - posed[0]).max()))
            if O[0] > 0:
                s_o = max(s_o, abs(O[k] - O[0]) / O[0])
    return s_pts, s_o, agree, margin


# The sensitivity figure of each case as tests/test_overlay_cpu.py measures it (the larger of the difference in posed points, in A, and in
# relative final O_AB between the three variants of the restatement), recorded as measured and not rounded. A case's bar on the GPU is
# max(1e-12, 1000 S[case]).
S = {
    "ref1": 1.3322676295501878e-15,
    "ref2": 2.694067191555405e-12,
    "ref41": 1.0408451878163305e-09,
    "ref41_nodes": 9.494431907342005e-10,
    "ref64": 3.814548676928098e-11,
    "ref65": 1.16000098415725e-10,
    "ref256": 1.099387425540499e-08,
    "iter0": 8.664053363493002e-16,
    "iter1": 1.8207657603852567e-14,
}


def bar(name):
    return max(1e-12, 1000 * S[name])
