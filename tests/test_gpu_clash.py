"""`pmx_pose_clash` on the GPU (csrc/pmx_pocket.hip) against the NumPy restatement of tests/clash_ref.py: point mode over the shapes at which
the kernel's trips change, node mode on the golden sets' own poses, the crystal ligand of the 6OIM fixture, the strictness of the two
thresholds, statuses, repeatability, and the Python layer on top of it.

Bars. Integers (counts, atoms, fingerprints, statuses) must be equal. A penetration is a handful of float64 operations on numbers below
100: 1e-12 * max(1, |value|). The overlap is a float64 sum of fewer than 10^6 non-negative terms, summed in another order than the
restatement's: 1e-10 * overlap. A row's integers can only differ from the restatement's where a pair stands within rounding of a threshold,
so every test asserts the restatement's `margin` - the smallest |pen| and |d - contact| of the call - to be at least 1e-9 for every row;
the seeds are chosen so (checked on the CPU for the seeded cases). The strictness test puts pairs on the thresholds on purpose and has
exact arithmetic instead."""

import ctypes
from functools import lru_cache

import numpy as np
import pytest

import clash_ref
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

MARGIN = 1e-9
COUNTS = (0, 1, 2, 63, 64, 65, 130, 300)
POCKET_SIZES = (0, 1, 63, 64, 65, 497, 1000)


def random_rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(n, 3, 3)
    assert np.allclose(np.linalg.det(R), 1.0)
    return R


def random_pocket(n_atoms, seed):
    from pharmaconet_amd.pocket import PocketAtoms

    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-10, 10, size=(n_atoms, 3)).astype(np.float32)
    radius = rng.choice(np.array([1.47, 1.52, 1.55, 1.6, 1.7, 1.8, 1.98], np.float32), size=n_atoms)
    group = rng.integers(0, 300, size=n_atoms).astype(np.uint16)  # (256 .. 299: atoms of no group, like 0xFFFF)
    group[rng.random(n_atoms) < 0.1] = 0xFFFF
    return PocketAtoms.from_arrays(xyz, radius, group)


@lru_cache(maxsize=None)
def point_case(n_atoms, with_radii, seed=0):
    """97 rows of random points under random proper rotations against a random pocket, and the restatement of every row: computed once."""
    rng = np.random.default_rng(1000 * n_atoms + seed + (500 if with_radii else 0))
    n = 97
    counts = rng.choice(COUNTS, size=n)
    counts[: len(COUNTS)] = COUNTS  # (every count at least once)
    points = [rng.uniform(-8, 8, size=(int(m), 3)).astype(np.float32) for m in counts]
    radii = [rng.uniform(1.0, 2.0, size=int(m)).astype(np.float32) for m in counts] if with_radii else None
    R, t = random_rotations(rng, n), rng.uniform(-2, 2, size=(n, 3))
    pocket = random_pocket(n_atoms, 77 + n_atoms)
    ref = [clash_ref.clash_row(pocket.xyz, pocket.radius, pocket.group, points[i], radii[i] if with_radii else np.float32(1.25), R[i], t[i], 0.5, 4.5) for i in range(n)]
    return pocket, points, radii, R, t, ref


def close(got, want, rel):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    fin = np.isfinite(want)
    return np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]) and bool((np.abs(got[fin] - want[fin]) <= rel * np.maximum(1.0, np.abs(want[fin]))).all())


def check_report(rep, ref, tag):
    """Every row of `rep` against the restatement's rows `ref`; the figures are printed before they are asserted."""
    assert len(rep) == len(ref), tag
    margin = min([r["margin"] for r in ref], default=np.inf)
    worst_pen = worst_ov = 0.0
    for i, r in enumerate(ref):
        fin = np.isfinite(r["point_pen"])
        if fin.any() and r["status"] == 0:
            worst_pen = max(worst_pen, float((np.abs(rep.point_penetration[i][fin] - r["point_pen"][fin]) / np.maximum(1.0, np.abs(r["point_pen"][fin]))).max()))
        if r["status"] == 0 and r["overlap"] > 0:
            worst_ov = max(worst_ov, abs(rep.overlap[i] - r["overlap"]) / r["overlap"])
    print(f"{tag}: rows {len(ref)} margin {margin:.3e} worst pen error {worst_pen:.3e} (bar 1e-12) worst overlap error {worst_ov:.3e} (bar 1e-10)")
    assert margin >= MARGIN, (tag, margin)
    for i, r in enumerate(ref):
        where = (tag, i)
        assert rep.status[i] == r["status"], where
        got = [rep.n_points[i], rep.n_clashing[i], rep.n_pairs[i], rep.n_contacts[i], rep.worst[i, 0], rep.worst[i, 1]]
        assert [int(v) for v in got] == r["counts"].tolist(), (where, got, r["counts"])
        assert np.array_equal(rep.point_atom[i], r["point_atom"]), where
        assert np.array_equal(rep.contact_fingerprint[i], r["fingerprint"]), where
        assert close(rep.point_penetration[i], r["point_pen"], 1e-12), where
        assert close(rep.clearance[i], r["clearance"], 1e-12), (where, rep.clearance[i], r["clearance"])
        if r["status"] == 0:
            assert abs(rep.overlap[i] - r["overlap"]) <= 1e-10 * r["overlap"], (where, rep.overlap[i], r["overlap"])
        else:
            assert np.isnan(rep.overlap[i]), where


def same_bits(a, b, rows=None):
    """Report `a` equals report `b` (its rows `rows`) bit for bit."""
    rows = np.arange(len(b)) if rows is None else np.asarray(rows)
    eq = lambda x, y: np.array_equal(x, y, equal_nan=True)  # noqa: E731
    return (len(a) == len(rows) and all(eq(getattr(a, f), getattr(b, f)[rows]) for f in ("clearance", "overlap", "n_points", "n_clashing", "n_pairs", "n_contacts", "worst",
                                                                                         "contact_fingerprint", "status"))
            and all(eq(a.point_penetration[k], b.point_penetration[j]) and eq(a.point_atom[k], b.point_atom[j]) for k, j in enumerate(rows)))


@lru_cache(maxsize=None)
def pocket_6oim(water=False):
    from pharmaconet_amd.pocket import PocketAtoms

    model, _, _, _ = load_golden("set_6oim_c8")
    return PocketAtoms.from_pdb(GOLDEN / "pocket_6oim.pdb", centers=model.node_centers, water=water)


@lru_cache(maxsize=None)
def crystal_ligand():
    from pharmaconet_amd.pocket import element_radii, parse_pdb_atoms

    lig = parse_pdb_atoms((GOLDEN / "ligand_6oim_mov.pdb").read_text())
    return lig, element_radii(lig.element)


# ---------------------------------------------------------------------------------------------------------------- 1. point mode
@pytest.mark.parametrize("with_radii", [False, True])
@pytest.mark.parametrize("n_atoms", POCKET_SIZES)
def test_point_mode_against_the_restatement(n_atoms, with_radii):
    from pharmaconet_amd.engine import clashes

    pocket, points, radii, R, t, ref = point_case(n_atoms, with_radii)
    rep = clashes(pocket, rotation=R, translation=t, points=points, point_radii=radii, node_radius=1.25)
    check_report(rep, ref, f"points, {n_atoms} atoms, radii {with_radii}")
    assert sorted(set(int(v) for v in rep.n_points)) == sorted(COUNTS)
    if n_atoms >= 497:
        assert (rep.n_pairs > 0).any() and (rep.n_contacts > 0).any() and rep.contact_fingerprint.any()
    if n_atoms == 0:
        assert np.isneginf(rep.clearance).all() and (rep.worst == -1).all() and not rep.contact_fingerprint.any()


# ---------------------------------------------------------------------------------------------------------------- 2. node mode
@pytest.mark.parametrize("name", ["set_6oim_c8", "set_6oim_c64", "set_s64_c8"])
def test_node_mode_on_the_sets_own_poses(name):
    from pharmaconet_amd.engine import clashes
    from test_gpu_align import posed

    model, lib, weights, ex, al = posed(name)
    pocket = pocket_6oim()
    rep = al.clashes(pocket, lib)
    nodes = [lib.unpack(int(i))["xyz"][:, :, int(c)].astype(np.float32) for i, c in zip(al.indices, al.conformers)]
    ok = al.status == 0
    assert ok.sum() >= 16 and (name != "set_s64_c8" or max(len(x) for x in nodes) == 64) and (name != "set_6oim_c64" or lib.headers()[:, 1].max() == 64)
    ref = [clash_ref.clash_row(pocket.xyz, pocket.radius, pocket.group, nodes[r], np.float32(1.0), al.rotation[r], al.translation[r]) for r in range(len(al))]
    check_report(rep, ref, f"nodes, {name}")
    assert np.array_equal(rep.status == 0, ok)
    if "6oim" in name:
        assert (rep.n_contacts[ok] > 0).any()  # the model is in the crystal frame: its poses land in the pocket
    # the same float32 positions as points: the same bits
    as_points = clashes(pocket, rotation=al.rotation, translation=al.translation, points=nodes, node_radius=1.0)
    assert same_bits(as_points, rep)


# ---------------------------------------------------------------------------------------------------------------- 3. the crystal ligand
def test_crystal_ligand_clashes_only_at_its_covalent_bond():
    from pharmaconet_amd.engine import clashes

    lig, radii = crystal_ligand()
    rng = np.random.default_rng(5)
    R, t = random_rotations(rng, 1)[0], rng.uniform(-20, 20, size=3)
    moved = ((lig.xyz.astype(np.float64) - t) @ R).astype(np.float32)  # x' = R^T (x - t): the motion (R, t) brings it back, to float32 rounding
    for water in (False, True):
        pocket = pocket_6oim(water)
        rep = clashes(pocket, rotation=[np.eye(3), R], translation=[np.zeros(3), t], points=[lig.xyz, moved], point_radii=[radii, radii])
        ref = [clash_ref.clash_row(pocket.xyz, pocket.radius, pocket.group, p, radii, Rk, tk) for p, Rk, tk in ((lig.xyz, np.eye(3), np.zeros(3)), (moved, R, t))]
        check_report(rep, ref, f"crystal ligand, water {water}")
        for i in range(2):
            assert (int(rep.n_points[i]), int(rep.n_clashing[i]), int(rep.n_pairs[i])) == (41, 2, 2) and rep.status[i] == 0
            assert lig.name[int(rep.worst[i, 0])] == "C25" and rep.atom_label(i, pocket) == "A:CYS12:SG"
            clashing = np.flatnonzero(rep.point_penetration[i] > 0)
            assert sorted(lig.name[clashing]) == ["C24", "C25"] and {pocket.atom_label(int(a)) for a in rep.point_atom[i][clashing]} == {"A:CYS12:SG"}
            assert "A:CYS12" in rep.residues(i, pocket)
            assert abs(rep.clearance[i] - 1.1946) < (5e-5 if i == 0 else 1e-4) and abs(rep.overlap[i] - 1.4930) < (5e-5 if i == 0 else 1e-4)
            assert int(rep.n_contacts[i]) == 39 if not water else int(rep.n_contacts[i]) >= 39
        assert rep.ok().tolist() == [False, False] and rep.ok(max_clashing=2).tolist() == [True, True]


# ---------------------------------------------------------------------------------------------------------------- 4. strictness
def test_thresholds_are_strict():
    """s = (1.5 + 1.0) - 0.5 = 2 exactly: a point at distance 2 has pen == 0 and does not clash, one float32 step closer it does. The same
    for the contact distance 4.5. Every number is exact in float32 and float64, so there is no margin to ask for."""
    from pharmaconet_amd.engine import clashes
    from pharmaconet_amd.pocket import PocketAtoms

    pocket = PocketAtoms.from_arrays([[0, 0, 0]], [1.5], [7])
    inside2, inside45 = np.nextafter(np.float32(2), np.float32(0)), np.nextafter(np.float32(4.5), np.float32(0))
    pts = [np.array([[2, 0, 0]], np.float32), np.array([[inside2, 0, 0]], np.float32), np.array([[0, 4.5, 0]], np.float32), np.array([[0, inside45, 0]], np.float32)]
    rep = clashes(pocket, rotation=[np.eye(3)] * 4, translation=[np.zeros(3)] * 4, points=pts, node_radius=1.0, tolerance=0.5, contact=4.5)
    assert rep.status.tolist() == [0] * 4
    assert rep.clearance[0] == 0.0 and rep.n_pairs.tolist() == [0, 1, 0, 0] and rep.n_clashing.tolist() == [0, 1, 0, 0]
    assert rep.clearance[1] == 2.0 - float(inside2) > 0 and rep.overlap[1] == (2.0 - float(inside2)) ** 2 and rep.overlap[0] == 0.0
    assert rep.n_contacts.tolist() == [1, 1, 0, 1]
    assert [int(fp[0]) for fp in rep.contact_fingerprint] == [1 << 7, 1 << 7, 0, 1 << 7] and not rep.contact_fingerprint[:, 1:].any()
    assert rep.worst.tolist() == [[0, 0]] * 4 and rep.clearance[2] == -2.5


# ---------------------------------------------------------------------------------------------------------------- 5. statuses
def raw_call(pocket, n=1, lib=None, node=False, pts=False, null=()):
    """pmx_pose_clash itself with one identity row: `node` / `pts` say which sources are given, `null` which outputs are withheld. The return code."""
    import torch

    from pharmaconet_amd import _ffi
    from pharmaconet_amd.engine import device_pocket

    dev = torch.device("cuda", torch.cuda.current_device())
    ph = device_pocket(pocket, dev.index)
    f64 = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)  # noqa: E731
    lig, conf = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    off, xyz = torch.tensor([0, 1], dtype=torch.int64, device=dev), torch.zeros((1, 3), dtype=torch.float32, device=dev)
    rot, trans = f64(np.eye(3).reshape(1, 9)), f64(np.zeros((1, 3)))
    out = dict(summary=torch.empty((1, 4), dtype=torch.float64, device=dev), count=torch.empty((1, 6), dtype=torch.int32, device=dev),
               ppen=torch.empty(64, dtype=torch.float64, device=dev), patom=torch.empty(64, dtype=torch.int32, device=dev),
               fp=torch.empty((1, 4), dtype=torch.int64, device=dev), status=torch.empty(1, dtype=torch.int32, device=dev))
    ptr = {k: (None if k in null else v.data_ptr()) for k, v in out.items()}
    stream = torch.cuda.current_stream(dev)
    rc = _ffi.load().pmx_pose_clash(ph.handle, lib.handle if node else None, lig.data_ptr() if node else None, conf.data_ptr() if node else None,
                                    off.data_ptr() if pts else None, xyz.data_ptr() if pts else None, None, rot.data_ptr(), trans.data_ptr(), n, 1.0, 0.5, 4.5,
                                    ptr["summary"], ptr["count"], ptr["ppen"], ptr["patom"], ptr["fp"], ptr["status"], ctypes.c_void_p(stream.cuda_stream))
    stream.synchronize()
    return rc, out


def test_statuses_and_refused_calls():
    from pharmaconet_amd.engine import DeviceLibrary, align, clashes

    model, lib, weights, _ = load_golden("set_6oim_c8")
    pocket = pocket_6oim()
    C = int(lib.header(0)[1])
    eye, zero = np.eye(3), np.zeros(3)
    bad_r, bad_t = eye.copy(), zero.copy()
    bad_r[1, 2], bad_t[0] = np.nan, np.inf
    idx = [len(lib), 0, 0, 0, 0, 0, len(lib) + 10**9]
    conf = [0, C, -1, 0, 0, 0, 0]
    rot = [eye, eye, eye, bad_r, eye, eye, eye]
    trans = [zero, zero, zero, zero, bad_t, zero, zero]
    rep = clashes(pocket, library=lib, indices=idx, conformers=conf, rotation=rot, translation=trans)
    assert rep.status.tolist() == [1, 4, 4, 4, 4, 0, 1]
    n0 = int(lib.header(0)[0])
    for i in (0, 1, 2, 3, 4, 6):
        assert np.isnan(rep.clearance[i]) and np.isnan(rep.overlap[i]) and rep.worst[i].tolist() == [-1, -1] and not rep.contact_fingerprint[i].any()
        assert (rep.n_points[i], rep.n_clashing[i], rep.n_pairs[i], rep.n_contacts[i]) == (0, 0, 0, 0)
        assert len(rep.point_penetration[i]) == (0 if rep.status[i] == 1 else n0) and np.isnan(rep.point_penetration[i]).all() and (rep.point_atom[i] == -1).all()
    ref = clash_ref.clash_row(pocket.xyz, pocket.radius, pocket.group, lib.unpack(0)["xyz"][:, :, 0], np.float32(1.0), eye, zero)
    assert ref["margin"] >= MARGIN and rep.n_points[5] == n0 and [int(v) for v in (rep.n_clashing[5], rep.n_pairs[5], rep.n_contacts[5])] == ref["counts"][1:4].tolist()
    # point mode: a motion that is not finite
    pm = clashes(pocket, rotation=[bad_r, eye], translation=[zero, zero], points=[np.zeros((3, 3)), np.zeros((2, 3))])
    assert pm.status.tolist() == [4, 0] and np.isnan(pm.point_penetration[0]).all() and len(pm.point_penetration[0]) == 3 and pm.n_points.tolist() == [0, 2]
    # a row of an Alignment that is not OK passes through with its status
    al = align(model, lib, [0, 1], [0, C + 3], [[-1], [-1]], weights=weights)
    assert al.status.tolist() == [0, 4]
    through = al.clashes(pocket, lib)
    assert through.status.tolist() == [0, 4] and np.isnan(through.clearance[1]) and through.ok().tolist()[1] is False
    # n = 0
    empty = clashes(pocket, library=lib, indices=[], conformers=[], rotation=np.zeros((0, 3, 3)), translation=np.zeros((0, 3)))
    assert len(empty) == 0 and empty.contact_fingerprint.shape == (0, 4) and clashes(pocket, rotation=[], translation=[], points=[]).status.shape == (0,)
    # both point sources, or neither; null outputs: refused, nothing runs
    with pytest.raises(ValueError):
        clashes(pocket, library=lib, indices=[0], conformers=[0], rotation=[eye], translation=[zero], points=[np.zeros((1, 3))])
    with pytest.raises(ValueError):
        clashes(pocket, rotation=[eye], translation=[zero])
    dlib = DeviceLibrary(lib)
    assert raw_call(pocket, lib=dlib, node=True, pts=True)[0] == 1 and raw_call(pocket)[0] == 1
    assert raw_call(pocket, n=0, lib=dlib, node=True, pts=True)[0] == 1 and raw_call(pocket, n=0, pts=True)[0] == 0 and raw_call(pocket, n=65537, pts=True)[0] == 1
    for name in ("summary", "count", "ppen", "patom", "status"):
        assert raw_call(pocket, pts=True, null=(name,))[0] == 1, name
        assert raw_call(pocket, lib=dlib, node=True, null=(name,))[0] == 1, name
    rc, out = raw_call(pocket, pts=True, null=("fp",))  # (the fingerprint alone may be withheld)
    assert rc == 0 and int(out["status"].cpu()[0]) == 0 and int(out["count"].cpu()[0, 0]) == 1
    rc, out = raw_call(pocket, lib=dlib, node=True)
    assert rc == 0 and int(out["status"].cpu()[0]) == 0
    dlib.close()


# ---------------------------------------------------------------------------------------------------------------- 6. repeatability
def test_same_bits_twice_and_under_a_permutation_of_the_rows():
    from pharmaconet_amd.engine import clashes

    pocket, points, radii, R, t, ref = point_case(497, True)
    assert min(r["margin"] for r in ref) >= MARGIN
    a = clashes(pocket, rotation=R, translation=t, points=points, point_radii=radii, node_radius=1.25)
    b = clashes(pocket, rotation=R, translation=t, points=points, point_radii=radii, node_radius=1.25)
    assert same_bits(a, b)
    perm = np.random.default_rng(3).permutation(len(points))
    c = clashes(pocket, rotation=R[perm], translation=t[perm], points=[points[j] for j in perm], point_radii=[radii[j] for j in perm], node_radius=1.25)
    assert same_bits(c, a, rows=perm)


# ---------------------------------------------------------------------------------------------------------------- 7. the Python layer
def test_alignment_clashes_in_both_levels_and_scoring_clash():
    from pharmaconet_amd.engine import clashes, fingerprint_similarity
    from pharmaconet_amd.pocket import atomic_number_radii
    from test_attribution_cpu import load_mols
    from test_gpu_align import posed

    model, lib, weights, ex, al = posed("set_6oim_c8")
    mols = load_mols("set_6oim_c8")
    pocket = pocket_6oim()
    nodes = al.clashes(pocket, lib)
    direct = clashes(pocket, library=lib, indices=al.indices, conformers=al.conformers, rotation=al.rotation, translation=al.translation)
    assert same_bits(nodes, direct) and len(nodes) == len(al)
    atoms = al.clashes(pocket, atoms=[mols[int(i)] for i in al.indices])
    ref = []
    for r, i in enumerate(al.indices):
        z = np.asarray(mols[int(i)].atomic_nums)
        pos = np.asarray(mols[int(i)].atom_positions, dtype=np.float32)[z > 1, int(al.conformers[r])]
        ref.append(clash_ref.clash_row(pocket.xyz, pocket.radius, pocket.group, pos, atomic_number_radii(z[z > 1]), al.rotation[r], al.translation[r]))
    check_report(atoms, ref, "Alignment.clashes(atoms=)")
    assert (atoms.n_points >= nodes.n_points).any()
    # the report's similarity is the fingerprint call on its words
    assert np.array_equal(atoms.similarity(), fingerprint_similarity(atoms.contact_fingerprint)) and atoms.similarity().shape == (len(al), len(al))
    assert np.array_equal(atoms.similarity(nodes), fingerprint_similarity(atoms.contact_fingerprint, nodes.contact_fingerprint))
    leaders, leader_of = atoms.leaders(threshold=0.5)
    assert leaders[0] == 0 and len(leader_of) == len(al)
    # one ligand
    r = next(r for r in range(len(al)) if al.n_nodes[r] >= 3)
    i = int(al.indices[r])
    one = model.scoring_clash(mols[i], weights=weights, pocket=pocket)
    assert one["level"] == "atoms" and one["status"] == 0 and one["conformer"] == al.conformers[r] and np.array_equal(one["rotation"], al.rotation[r])
    assert (one["clearance"], one["overlap"], one["n_points"], one["n_clashing"], one["n_pairs"], one["n_contacts"]) == (
        atoms.clearance[r], atoms.overlap[r], atoms.n_points[r], atoms.n_clashing[r], atoms.n_pairs[r], atoms.n_contacts[r])
    assert np.array_equal(one["point_penetration"], atoms.point_penetration[r]) and one["residues"] == atoms.residues(r, pocket) and one["ok"] == bool(atoms.ok()[r])
    assert one["worst_atom"] == atoms.atom_label(r, pocket)
    packed = model.scoring_clash(lib.record(i), weights=weights, pocket=pocket)
    assert packed["level"] == "nodes" and packed["n_points"] == nodes.n_points[r] and packed["clearance"] == nodes.clearance[r]
    with pytest.raises(ValueError, match="no ATOM / HETATM record"):
        model.scoring_clash(mols[i], weights=weights)  # (the golden model carries no protein)


def test_fitting_keeps_rank_order_and_returns_passing_rows_only():
    model, lib, weights, _ = load_golden("set_6oim_c8")
    pocket = pocket_6oim()
    lib = lib.select(np.arange(24))
    res = model.screen(lib, weights=weights)
    pool = 16
    seen = set()
    for max_clashing in (0, 2, 64):
        fit = res.fitting(5, pool=pool, max_clashing=max_clashing, pocket=pocket)
        rep, al = fit.report, fit.poses
        passes = rep.ok(max_clashing) & (al.status == 0)
        want = np.flatnonzero(passes)[:5]
        assert np.array_equal(fit.rows, want) and np.array_equal(fit.indices, al.indices[want].astype(np.uint64)) and len(fit) == len(want)
        assert (np.diff(fit.ranks) > 0).all() and (rep.status[fit.rows] == 0).all() and (rep.n_clashing[fit.rows] <= max_clashing).all()
        assert np.array_equal(fit.pool, res._best(pool)) and np.array_equal(fit.pool[fit.ranks], fit.indices)
        seen.add(len(fit))
    assert 5 in seen  # (with 64 clashing points allowed every posed hit passes)
    with pytest.raises(ValueError):
        res.fitting(0, pocket=pocket)


def test_cli_clashes_csv(tmp_path):
    from pharmaconet_amd.engine import explain
    from pharmaconet_amd.screening import main

    model, lib, _, _ = load_golden("set_6oim_c8")
    pocket = pocket_6oim()
    lib = lib.select(np.arange(16))  # (a screen of 16 ligands: the command line is what is tested)
    libfile = tmp_path / "lib.pmxlib"
    lib.save(libfile)
    args = ["-p", str(GOLDEN / "model_6oim_like.pm"), "-d", str(libfile), "--explain", "5"]
    clash = ["--clashes", str(tmp_path / "clashes.csv"), "--protein", str(GOLDEN / "pocket_6oim.pdb"), "--clash_level", "nodes"]
    main(args + ["-o", str(tmp_path / "plain.csv"), "--explain_out", str(tmp_path / "plain_hits.csv"), "--poses", str(tmp_path / "plain_poses.csv")])
    main(args + ["-o", str(tmp_path / "with.csv"), "--explain_out", str(tmp_path / "hits.csv"), "--poses", str(tmp_path / "poses.csv")] + clash)
    for a, b in (("plain.csv", "with.csv"), ("plain_hits.csv", "hits.csv"), ("plain_poses.csv", "poses.csv")):
        assert (tmp_path / a).read_bytes() == (tmp_path / b).read_bytes()
    base = ["-p", str(GOLDEN / "model_6oim_like.pm"), "-d", str(libfile), "-o", str(tmp_path / "x.csv")]
    for bad in (clash, ["--explain", "5", "--clashes", str(tmp_path / "c.csv"), "--protein", str(GOLDEN / "pocket_6oim.pdb")],  # no --explain; atoms of a packed library
                ["--explain", "5", "--clashes", str(tmp_path / "c.csv"), "--clash_level", "nodes"],  # the golden model carries no protein
                ["--explain", "5", "--protein", str(GOLDEN / "pocket_6oim.pdb")]):
        with pytest.raises(SystemExit):
            main(base + bad)
    hits = [row.split(",") for row in (tmp_path / "hits.csv").read_text().splitlines()[1:]]
    rows = (tmp_path / "clashes.csv").read_text().splitlines()
    assert rows[0] == "rank,path,conformer,level,points,clashing,pairs,clearance,overlap,contacts,worst_point,worst_atom,residues" and len(rows) == len(hits) + 1 == 6
    names = {f"{libfile}#{i}": i for i in range(len(lib))}
    idx = [names[h[1]] for h in hits]
    rep = explain(model, lib, idx).poses(model, lib).clashes(pocket, lib)  # (the command line's default weights are the engine's)
    for r, row in enumerate(rows[1:]):
        f = row.split(",")
        assert len(f) == 13 and int(f[0]) == r + 1 and f[1] == hits[r][1] and int(f[2]) == int(hits[r][3]) and f[3] == "nodes"
        assert [int(f[4]), int(f[5]), int(f[6]), int(f[9]), int(f[10])] == [int(v) for v in (rep.n_points[r], rep.n_clashing[r], rep.n_pairs[r], rep.n_contacts[r], rep.worst[r, 0])]
        assert float(f[7]) == rep.clearance[r] and float(f[8]) == rep.overlap[r] and repr(float(f[7])) == f[7]
        assert f[11] == rep.atom_label(r, pocket) and f[12] == ";".join(rep.residues(r, pocket))
