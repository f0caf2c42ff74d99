"""The atom store on the GPU (csrc/pmx_atoms.hip, `pmx_pose_search_atoms` in csrc/pmx_pose_search.hip; the definitions are the comments of
include/pmx.h).

`pmx_atoms_gather` copies: against tests/atoms_ref.py every coordinate, radius, offset and status must be the same bits. The store is a
second way to the rows `Alignment.clashes(atoms=[molecules])` already makes on the host, so every field of the reports of the two ways
must be the same bits too. The atom-level search composes `align`, the gather and `clashes` with the unchanged rule: its choices must be
those of the NumPy chain of tests/test_atoms_cpu.py (which asserts that no decision of that chain stands within 1e-9 of a threshold), its
poses those of `align`, its report that of `clashes(atoms=store)`, bit for bit."""

from functools import lru_cache

import numpy as np
import pytest

import atoms_ref
import pose_search_ref as psr
from conftest import GOLDEN, load_golden
from test_attribution_cpu import load_mols

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 255, 256)  # atoms per record: around the trips of 64 lanes, and the limit
CONFS = (1, 8, 64)


@lru_cache(maxsize=None)
def pocket_6oim():
    from pharmaconet_amd.pocket import PocketAtoms

    model, _, _, _ = load_golden("set_6oim_c8")
    return PocketAtoms.from_pdb(GOLDEN / "pocket_6oim.pdb", centers=model.node_centers)


@lru_cache(maxsize=None)
def store_6oim():
    """The atom store of set_6oim_c8 and the molecules it was made from: built once, shared, never written to."""
    from pharmaconet_amd.atoms import PackedAtoms

    _, lib, _, _ = load_golden("set_6oim_c8")
    mols = load_mols("set_6oim_c8")
    return PackedAtoms.for_library(mols, lib), mols


# ---------------------------------------------------------------------------------------------------------------- 1. the gather
@lru_cache(maxsize=None)
def edge_store():
    """21 records: every size of SIZES at every conformer count of CONFS, heavy elements of several radii with hydrogens in between."""
    rng = np.random.default_rng(3)
    zs, ps = [], []
    for n in SIZES:
        for C in CONFS:
            z = rng.choice([6, 7, 8, 9, 15, 16, 17, 35, 53, 5], size=n)
            z = np.insert(z, rng.integers(0, n + 1, size=3), 1)  # three hydrogens somewhere
            zs.append(z.astype(np.int64))
            ps.append(rng.normal(scale=8.0, size=(len(z), C, 3)).astype(np.float32))
    return zs, ps


def edge_rows():
    """97 rows: every record at conformer 0, its last, -1 and n_conf; an index one past the store, twice; repeats."""
    lig, conf = [], []
    for i in range(len(SIZES) * len(CONFS)):
        C = CONFS[i % len(CONFS)]
        lig += [i, i, i, i]
        conf += [0, C - 1, -1, C]
    lig += [21, 21] + [20, 20, 20, 5, 5, 13, 13, 13, 13, 9, 2]
    conf += [0, -1] + [63, 63, 0, 7, 7, 0, 0, 0, 7, 0, 63]
    assert len(lig) == 97
    return np.array(lig, np.int64), np.array(conf, np.int64)


def check_gather(dat, off, data, table, lig, conf, tag):
    got = dat.gather(lig, conf)
    want = atoms_ref.gather(off, data, table, lig, conf)
    for g, w, name in zip(got, want, ("point_off", "points", "radii", "status")):
        assert g.shape == w.shape and g.tobytes() == w.astype(g.dtype).tobytes(), (tag, name)
    return got


def test_gather_equals_the_restatement_bit_for_bit():
    from pharmaconet_amd.atoms import PackedAtoms
    from pharmaconet_amd.engine import DeviceAtoms
    from pharmaconet_amd.pocket import atomic_number_radii

    zs, ps = edge_store()
    st = PackedAtoms.from_arrays(zs, ps)
    off, data = atoms_ref.store(zs, ps)
    assert np.array_equal(st.offsets, off) and st.data.tobytes() == data.tobytes()
    table = atomic_number_radii(np.arange(128))
    dat = DeviceAtoms(st)
    assert (len(dat), dat.num_bytes, dat.max_atoms, dat.num_empty) == (21, int(off[-1]), 256, 3)
    lig, conf = edge_rows()
    po, pts, rad, status = check_gather(dat, off, data, table, lig, conf, "97 rows")
    assert (status == 0).sum() == 2 * 18 + 10 and (status == 1).sum() == 4 * 3 + 3 and (status == 4).sum() == 2 * 18  # (every kind of row is there)
    assert len(set(np.unique(rad).tolist())) >= 5 and int(po[-1]) == len(pts) > 97 * 40
    check_gather(dat, off, data, table, lig[:0], conf[:0], "0 rows")
    for r in (0, 5, 80, 84, 96):
        check_gather(dat, off, data, table, lig[r: r + 1], conf[r: r + 1], f"row {r} alone")
    # the same rows in another order: each row has the contents it had
    perm = np.random.default_rng(8).permutation(97)
    po2, pts2, rad2, status2 = dat.gather(lig[perm], conf[perm])
    assert np.array_equal(status2, status[perm])
    for k, r in enumerate(perm):
        a, b = slice(po2[k], po2[k + 1]), slice(po[r], po[r + 1])
        assert pts2[a].tobytes() == pts[b].tobytes() and rad2[a].tobytes() == rad[b].tobytes(), (k, r)
    again = dat.gather(lig, conf)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(again, (po, pts, rad, status)))  # two runs, the same bits
    # a store without an atom, and an empty one
    none = DeviceAtoms(PackedAtoms.from_arrays([[1, 1], []], [np.zeros((2, 1, 3), np.float32), np.zeros((0, 1, 3), np.float32)]))
    assert (none.max_atoms, none.num_empty) == (0, 2)
    po0, pts0, _, st0 = none.gather([0, 1, 2], [0, 0, 0])
    assert po0.tolist() == [0, 0, 0, 0] and len(pts0) == 0 and st0.tolist() == [1, 1, 1]
    empty = DeviceAtoms(PackedAtoms.from_arrays([], []))
    assert len(empty) == 0 and empty.gather([0], [0])[3].tolist() == [1]
    for d in (dat, none, empty):
        d.close()
    with pytest.raises(Exception):
        dat.gather([0], [0])


# ---------------------------------------------------------------------------------------------------------------- 2. the store against the molecules
def test_clashes_and_refine_from_the_store_equal_the_list_of_molecules():
    from pharmaconet_amd.engine import align, clashes
    from test_gpu_align import posed
    from test_gpu_clash import same_bits as same_report
    from test_gpu_refine import same_bits as same_refined

    model, lib, weights, ex, al = posed("set_6oim_c8")
    pocket = pocket_6oim()
    st, mols = store_6oim()
    listed = [mols[int(i)] for i in al.indices]
    want = al.clashes(pocket, atoms=listed)
    assert (want.status == 0).sum() >= 16 and (want.n_points[want.status == 0] > 0).all()
    with _resident(st) as dat:
        for source in (st, dat):  # a host store is uploaded for the call; a resident one is used as it is
            assert same_report(al.clashes(pocket, atoms=source), want)
            assert same_report(clashes(pocket, atoms=source, indices=al.indices, conformers=al.conformers, rotation=al.rotation, translation=al.translation), want)
        ref_want = al.refine(pocket, atoms=listed)
        ref = al.refine(pocket, atoms=dat)
        assert same_refined(ref, ref_want) and np.array_equal(ref.indices, ref_want.indices)
        assert same_report(ref.clashes(pocket, atoms=dat), ref_want.clashes(pocket, atoms=listed))
        # rows that are not OK: a conformer the molecule lacks, and none - the status comes through both ways
        rows, conf, keys = ex._own_rows(None)
        rows, conf, keys = rows[:6], list(conf[:6]), keys[:6]
        conf[1], conf[4] = 8, -1
        idx = [int(ex.indices[r]) for r in rows]
        bad = align(model, lib, idx, conf, keys, weights=weights)
        assert bad.status[[1, 4]].tolist() == [4, 4] and (bad.status[[0, 2, 3, 5]] == 0).all()
        a, b = bad.clashes(pocket, atoms=dat), bad.clashes(pocket, atoms=[mols[i] for i in idx])
        assert same_report(a, b) and np.array_equal(a.status, bad.status) and np.isnan(a.overlap[1]) and a.n_points[4] == 0
        assert same_refined(bad.refine(pocket, atoms=dat), bad.refine(pocket, atoms=[mols[i] for i in idx]))
        # what only the store can say: a ligand it has no atoms for, a finite motion on a conformer that is none
        eye, zero = np.broadcast_to(np.eye(3), (3, 3, 3)), np.zeros((3, 3))
        odd = clashes(pocket, atoms=dat, indices=[0, len(st), 0], conformers=[0, 0, 8], rotation=eye, translation=zero)
        assert odd.status.tolist() == [0, 1, 4] and np.isnan(odd.clearance[1:]).all() and odd.n_points.tolist()[1:] == [0, 0] and odd.worst[1:].tolist() == [[-1, -1]] * 2
    with pytest.raises(ValueError, match="one source"):
        clashes(pocket, library=lib, atoms=st, indices=[0], conformers=[0], rotation=np.eye(3)[None], translation=np.zeros((1, 3)))


def _resident(st):
    from pharmaconet_amd.engine import _device_index, _resident_atoms

    return _resident_atoms(st, _device_index(None))


# ---------------------------------------------------------------------------------------------------------------- 3. the search
@lru_cache(maxsize=None)
def searched():
    """The 13 fixture hits: their modes on the GPU, the node-level and the atom-level search, and the restated atom chain on the fits of
    tests/pose_search_ref.py - at the GPU's motion where the restatement's rotation is not unique. Computed once, shared, never written to."""
    import align_ref
    from explain_ref import Tables
    from pharmaconet_amd.constants import weights_vector
    from pharmaconet_amd.engine import align, explain_modes, pose_search
    from test_atoms_cpu import atom_choice
    from test_pose_search_cpu import fixture_chain

    model, lib, weights, _ = load_golden("set_6oim_c8")
    w7 = weights_vector(weights)
    pocket = pocket_6oim()
    st, mols = store_6oim()
    idx = [h["index"] for h in fixture_chain()]
    ms = explain_modes(model, lib, idx, modes=4, weights=weights)
    assert (ms.status == 0).all()
    slots = [(i, m, c) for i in range(len(idx)) for m in range(4) for c in range(8) if ms.values[i][m, c] > 0]
    al_all = align(model, lib, [idx[i] for i, _, _ in slots], [c for _, _, c in slots], [ms.match[i][m, c] for i, m, c in slots], weights=weights)
    Yc = align_ref.node_centers(model)
    rows, motions, loose = [{} for _ in idx], [{} for _ in idx], 0
    tables = [Tables(model, lib.unpack(lig), w7) for lig in idx]
    for row, (i, m, c) in enumerate(slots):
        s = rows[i][m, c] = psr.slot(model, lib.unpack(idx[i]), w7, pocket, ms.levels[i], ms.match[i][m, c], c, tables[i], Yc)
        if s["align_ok"] and not psr.unique(s["fit"]):  # (two correct fits pose differently: the check is made at the motion under test)
            loose += 1
            motions[i][m, c] = (al_all.rotation[row], al_all.translation[row])
    chain = [atom_choice(ms.values[i], rows[i], mols[lig], pocket, 4, 8, motions=motions[i]) for i, lig in enumerate(idx)]
    print(f"{len(slots)} slots, {loose} of them with a rotation that is not unique (checked at the GPU's motion)")
    nodes = pose_search(model, lib, pocket, idx, modes=4, weights=weights)
    atoms = pose_search(model, lib, pocket, idx, modes=4, weights=weights, atoms=st)
    return idx, ms, chain, nodes, atoms, motions


def test_search_on_atoms_equals_the_restated_chain():
    from pharmaconet_amd.engine import align, clashes, pose_search
    from test_gpu_clash import same_bits as same_report
    from test_gpu_pose_search import same_poses

    model, lib, weights, _ = load_golden("set_6oim_c8")
    pocket = pocket_6oim()
    st, mols = store_6oim()
    idx, ms, chain, nodes, ps, free = searched()
    assert len(idx) == 13 and ps.level == "atoms" and nodes.level == "nodes" and nodes.gather_status is None
    margin = min(r["margin"] for ref in chain for r in ref["atoms"].values())
    print(f"smallest clash margin over the atoms of the chain's candidate rows: {margin:.3g} (bar 1e-9)")
    assert margin >= 1e-9
    rep = ps.report()
    for i, (lig, ref) in enumerate(zip(idx, chain)):
        got = (int(ps.conformer[i]), int(ps.mode[i]), bool(ps.passes[i]), int(ps.n_candidates[i]), int(ps.n_passing[i]), int(ps.n_dropped[i]))
        want = (ref["conformer"], ref["mode"], ref["passes"], ref["n_candidates"], ref["n_passing"], ref["n_dropped"])
        print(f"ligand {lig}: GPU {got}, chain {want}; at node level {(int(nodes.conformer[i]), int(nodes.mode[i]), bool(nodes.passes[i]))}")
        assert got == want, lig
        assert ps.value[i] == ref["value"] and ps.fraction[i] == ref["fraction"], lig  # (equal as bits: the values are the GPU's own modes)
        cl = ref["atoms"][ref["mode"], ref["conformer"]]
        counts = [rep.n_points[i], rep.n_clashing[i], rep.n_pairs[i], rep.n_contacts[i], rep.worst[i, 0], rep.worst[i, 1]]
        assert int(rep.n_points[i]) == int((np.asarray(mols[lig].atomic_nums) > 1).sum()), lig
        assert [int(v) for v in counts] == cl["counts"].tolist(), (lig, counts, cl["counts"])
        assert np.array_equal(rep.point_atom[i], cl["point_atom"]) and np.array_equal(rep.contact_fingerprint[i], cl["fingerprint"]), lig
    # the poses are `align`'s and the report is `clashes(atoms=store)`'s of the chosen rows, bit for bit
    keys = [ms.match[i][ps.mode[i], ps.conformer[i]] for i in range(13)]
    al = align(model, lib, idx, ps.conformer, keys, weights=weights)
    assert same_poses(ps.alignment(), al) and (al.status == 0).all()
    assert same_report(rep, clashes(pocket, atoms=st, indices=idx, conformers=ps.conformer, rotation=al.rotation, translation=al.translation))
    assert same_report(rep, ps.alignment().clashes(pocket, atoms=[mols[i] for i in idx]))  # ... and the list of molecules'
    assert (ps.gather_status == 0).all() and (rep.status == 0).all()
    # what the feature is for: the atoms choose differently from the nodes, and find the two poses that pass
    differ = [lig for i, lig in enumerate(idx) if (nodes.conformer[i], nodes.mode[i]) != (ps.conformer[i], ps.mode[i])]
    passing = {lig: (int(ps.conformer[i]), int(ps.mode[i])) for i, lig in enumerate(idx) if ps.passes[i]}
    print(f"node level: {int(nodes.passes.sum())} of 13 pass; atom level: {passing}; another (conformer, mode) for {len(differ)} hits: {differ}")
    assert int(nodes.passes.sum()) == 7 and len(differ) == 8 and set(passing) == {121, 282} and passing[121] == (3, 0)
    # ligand 282: the chain of tests/test_atoms_cpu.py poses it at conformer 1 under mode 0, but that slot's fit has a free rotation (one
    # matched cluster: `pose_search_ref.unique`), NumPy's eigensolver takes one, `pmx_align` the identity, and only the first clears the
    # atoms. At the motion under test the best-scoring slot that passes is another - the chain's choice at that motion, asserted above
    r = idx.index(282)
    print(f"ligand 282: {int(chain[r]['n_passing'])} passing slots; (mode 0, conformer 1) has a free rotation: {(0, 1) in free[r]}, passes at the GPU's motion: "
          f"{bool(chain[r]['passing'][0, 1])}")
    assert (0, 1) in free[r] or chain[r]["passing"][0, 1]
    node_choice_atoms = nodes.alignment().clashes(pocket, atoms=st)
    print(f"poses the node-level search accepts whose atoms clash: {int((node_choice_atoms.n_clashing[nodes.passes] > 0).sum())} of {int(nodes.passes.sum())}")
    assert ps.passes[node_choice_atoms.ok(0)].all()  # a node-level choice whose atoms pass is a passing candidate of the atom-level search
    assert (node_choice_atoms.n_clashing[nodes.passes & ~ps.passes] > 0).all() and int((nodes.passes & ~ps.passes).sum()) == 5
    # two runs, the same bits
    again = pose_search(model, lib, pocket, idx, modes=4, weights=weights, atoms=st)
    for f in ("conformer", "mode", "passes", "n_candidates", "n_passing", "n_dropped", "value", "fraction", "status", "gather_status"):
        assert np.array_equal(getattr(ps, f), getattr(again, f), equal_nan=True), f
    assert same_poses(ps.alignment(), again.alignment()) and same_report(rep, again.report())
    # the modes already held, and the one-ligand form
    held = ms.pose_search(model, lib, pocket, weights=weights, atoms=st)
    assert np.array_equal(held.conformer, ps.conformer) and np.array_equal(held.mode, ps.mode) and same_report(held.report(), rep)
    r = idx.index(121)
    one = model.scoring_pose_search(mols[121], modes=4, weights=weights, pocket=pocket, level="atoms")
    assert (one["level"], one["conformer"], one["mode"], one["passes"], one["n_clashing"]) == ("atoms", 3, 0, True, 0) and one["overlap"] == rep.overlap[r]
    assert model.scoring_pose_search(mols[121], modes=4, weights=weights, pocket=pocket)["level"] == "nodes"


def test_search_skips_a_hit_without_atoms():
    from pharmaconet_amd.atoms import PackedAtoms
    from pharmaconet_amd.engine import pose_search

    model, lib, weights, _ = load_golden("set_6oim_c8")
    pocket = pocket_6oim()
    _, mols = store_6oim()
    idx, _, _, _, ps, _ = searched()
    keep = np.ones(len(lib), bool)
    keep[idx[2]] = keep[121] = False
    part = pose_search(model, lib, pocket, idx, modes=4, weights=weights, atoms=PackedAtoms.from_features(mols, keep))
    for r in (2, idx.index(121)):  # header-only: no choice, though the hit was scored (and 121 would pass)
        assert (part.conformer[r], part.mode[r], part.passes[r], part.n_candidates[r], part.n_passing[r], part.status[r]) == (-1, -1, False, 0, 0, 0)
        assert part.gather_status[r] == 1 and part.report().status[r] == 1 and part.alignment().status[r] == 4 and np.isnan(part.value[r])
        assert np.isnan(part.report().overlap[r]) and part.report().n_points[r] == 0 and len(part.report().point_penetration[r]) == 0
        assert not part.report().ok(10**6)[r]
    rest = [r for r in range(13) if r not in (2, idx.index(121))]
    assert np.array_equal(part.conformer[rest], ps.conformer[rest]) and np.array_equal(part.report().overlap[rest], ps.report().overlap[rest])
    with pytest.raises(ValueError, match="atom store of"):
        pose_search(model, lib, pocket, idx, modes=4, weights=weights, atoms=PackedAtoms.from_features(mols[:5]))


# ---------------------------------------------------------------------------------------------------------------- 4. fitting and the command line
def test_fitting_with_the_store_returns_only_hits_whose_atoms_pass():
    from test_gpu_pose_search import small_trees

    model, lib, weights, d = load_golden("set_6oim_c8")
    pocket = pocket_6oim()
    st, mols = store_6oim()
    sel = np.unique(np.concatenate([small_trees(d, 22), [121, 282]]))  # (the two ligands that have a pose whose atoms pass among them)
    sub, sub_atoms = lib.select(sel), st.select(sel)
    res = model.screen(sub, weights=weights)
    fit = res.fitting(len(sel), pool=len(sel), pocket=pocket, search=4, atoms=sub_atoms)
    listed = fit.poses.clashes(pocket, atoms=[mols[int(sel[i])] for i in fit.poses.indices])  # the check the next step would make
    passes = listed.ok(0) & (fit.poses.status == 0)
    print(f"fitting(search=4, atoms=store) over {len(sel)} ligands: {len(fit)} hits whose atoms pass")
    assert np.array_equal(fit.rows, np.flatnonzero(passes)) and len(fit) >= 2 and {121, 282} <= set(sel[fit.indices.astype(np.int64)].tolist())
    assert (listed.n_clashing[fit.rows] == 0).all() and np.array_equal(fit.report.n_clashing, listed.n_clashing) and np.array_equal(fit.report.overlap, listed.overlap, equal_nan=True)
    by_nodes = res.fitting(len(sel), pool=len(sel), pocket=pocket, search=4, atoms=lambda i: mols[int(sel[i])])  # the node-level search, checked on atoms afterwards
    assert set(by_nodes.indices.tolist()) <= set(fit.indices.tolist())
    plain = res.fitting(len(sel), pool=len(sel), pocket=pocket, atoms=sub_atoms)  # without the search: the store only feeds the check
    want = res.fitting(len(sel), pool=len(sel), pocket=pocket, atoms=lambda i: mols[int(sel[i])])
    assert np.array_equal(plain.indices, want.indices) and np.array_equal(plain.report.overlap, want.report.overlap, equal_nan=True)


def test_cli_checks_a_packed_library_at_atom_level(tmp_path):
    from pharmaconet_amd.atoms import PackedAtoms, atoms_path
    from pharmaconet_amd.engine import explain
    from pharmaconet_amd.screening import main
    from test_gpu_pose_search import small_trees

    model, lib, _, d = load_golden("set_6oim_c8")
    st, mols = store_6oim()
    sel = small_trees(d, 16)
    libfile = tmp_path / "lib.pmxlib"
    lib.select(sel).save(libfile)
    st.select(sel).save(atoms_path(libfile))
    args = ["-p", str(GOLDEN / "model_6oim_like.pm"), "-d", str(libfile), "-o", str(tmp_path / "out.csv"), "--explain", "5", "--protein", str(GOLDEN / "pocket_6oim.pdb")]
    main(args + ["--clashes", str(tmp_path / "clashes.csv"), "--clash_level", "atoms", "--refine_out", str(tmp_path / "refined.csv"), "--pose_search", str(tmp_path / "search.csv"),
                 "--pose_search_level", "atoms", "--save_top", "4", str(tmp_path / "top.pmxlib")])
    rows = [r.split(",") for r in (tmp_path / "clashes.csv").read_text().splitlines()]
    assert rows[0][:10] == "rank,path,conformer,level,points,clashing,pairs,clearance,overlap,contacts".split(",") and len(rows) == 6
    order = [int(r[1].rsplit("#", 1)[1]) for r in rows[1:]]
    sub = lib.select(sel)
    al = explain(model, sub, order).poses(model, sub)
    want = al.clashes(pocket_6oim(), atoms=[mols[int(sel[i])] for i in order], tolerance=0.5)
    for r, row in enumerate(rows[1:]):
        assert row[3] == "atoms" and [int(row[2]), int(row[4]), int(row[5]), int(row[6]), int(row[9])] == [al.conformers[r], want.n_points[r], want.n_clashing[r], want.n_pairs[r],
                                                                                                           want.n_contacts[r]], row
        assert float(row[7]) == want.clearance[r] and float(row[8]) == want.overlap[r], row  # (repr round-trips: the same float64)
    assert len((tmp_path / "refined.csv").read_text().splitlines()) == 6 and len((tmp_path / "search.csv").read_text().splitlines()) == 6
    # --save_top carries the store along: record k of the saved store is the k-th best hit's
    top = PackedAtoms.load(atoms_path(tmp_path / "top.pmxlib"))
    assert len(top) == 4 and [top.record(k) for k in range(4)] == [st.record(int(sel[i])) for i in order[:4]]
    # ... and --pose_search_level nodes is the default, byte for byte
    main(args + ["--pose_search", str(tmp_path / "a.csv")])
    main(args + ["--pose_search", str(tmp_path / "b.csv"), "--pose_search_level", "nodes"])
    assert (tmp_path / "a.csv").read_bytes() == (tmp_path / "b.csv").read_bytes() != (tmp_path / "search.csv").read_bytes()
