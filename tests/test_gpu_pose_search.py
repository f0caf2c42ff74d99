"""`pmx_pose_search` on the GPU (csrc/pmx_pose_search.hip; the definition is the comment of include/pmx.h, restated in
tests/pose_search_ref.py).

The call is a composition of two calls the library already has, and a rule on their outputs that compares float64 bits and integers only.
So the first bar is equality, bit for bit: `explain_modes`, then `align` and `clashes` on the same slots, then the rule in NumPy, must give
the search's every integer, key, value, motion, fit, penetration, fingerprint and status (`composition`). Against the NumPy chain
(align_ref, clash_ref, the rule) the choices and the integers must be equal - tests/test_pose_search_cpu.py asserts that no decision of
that chain on this fixture stands within 1e-9 of a threshold - and the floats agree within the bars of tests/test_gpu_align.py
(1e-10 E0 on sse) and tests/test_gpu_clash.py (1e-12 on penetrations, 1e-10 on the overlap)."""

import dataclasses
from functools import lru_cache

import numpy as np
import pytest

import pose_search_ref as psr
from conftest import GOLDEN, load_golden
from explain_ref import candidates, ligand_levels

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)


@lru_cache(maxsize=None)
def pocket_6oim():
    from pharmaconet_amd.pocket import PocketAtoms

    model, _, _, _ = load_golden("set_6oim_c8")
    return PocketAtoms.from_pdb(GOLDEN / "pocket_6oim.pdb", centers=model.node_centers)


def small_trees(d, k, cap=30000):
    """The first k ligands of a set whose tree has at most `cap` nodes (`n_tree` of the set's npz): `pmx_explain_modes` walks a tree to its
    end, and one ligand among the first 24 of set_6oim_c8 has 5.5e7 nodes - seconds a call, which says nothing about the search."""
    return np.flatnonzero(d["n_tree"] <= cap)[:k]


def same_poses(a, b):
    from test_gpu_align import same_bits

    return same_bits(a, b) and np.array_equal(a.indices, b.indices) and np.array_equal(a.conformers, b.conformers)


def composition(ms, ps, model, lib, pocket, weights, stride, max_clashing=0, min_fitted=1, min_fraction=0.0, tolerance=0.5, contact=4.5, node_radius=1.0, tag=""):
    """The search `ps` of the modes `ms` against the calls it is made of: `align` and `clashes` on every slot (hit, mode, conformer <
    stride), the rule in NumPy, and the two calls once more on the chosen rows. Returns the rule's answers."""
    from pharmaconet_amd.engine import align, clashes
    from test_gpu_clash import same_bits as same_report

    n, M = len(ms), ms.modes
    lig, conf, keys, pre = [], [], [], []
    for i in range(n):
        scored = ms.status[i] == 0
        v = np.zeros((M, stride))
        C = min(ms.values[i].shape[1], stride) if scored else 0
        if scored:
            v[:, :C] = ms.values[i][:, :C]
        positive = v > 0
        vbest = v[positive].max() if positive.any() else 0.0
        for m in range(M):
            for c in range(stride):
                worth = bool(positive[m, c]) and v[m, c] >= np.float64(min_fraction) * vbest
                lig.append(int(ms.indices[i]))
                conf.append(c if worth else -1)
                keys.append(ms.match[i][m, c] if worth else np.zeros(0, np.int64))
        pre.append(v)
    al = align(model, lib, lig, conf, keys, weights=weights)
    rep = clashes(pocket, library=lib, indices=lig, conformers=conf, rotation=al.rotation, translation=al.translation, node_radius=node_radius, tolerance=tolerance,
                  contact=contact)
    chosen, rules = [], []
    for i in range(n):
        rows = slice(i * M * stride, (i + 1) * M * stride)
        shape = (M, stride)
        r = psr.choose(pre[i], (al.status[rows] == 0).reshape(shape), al.n_nodes[rows].reshape(shape), (rep.status[rows] == 0).reshape(shape),
                       rep.n_clashing[rows].reshape(shape), rep.overlap[rows].reshape(shape), ms.status[i] == 0, max_clashing, min_fitted, min_fraction)
        rules.append(r)
        where = (tag, i, int(ms.indices[i]))
        got = (int(ps.conformer[i]), int(ps.mode[i]), bool(ps.passes[i]), int(ps.n_candidates[i]), int(ps.n_passing[i]), int(ps.n_dropped[i]))
        assert got == (r["conformer"], r["mode"], r["passes"], r["n_candidates"], r["n_passing"], r["n_dropped"]), (where, got, r)
        assert np.array_equal([ps.value[i], ps.fraction[i]], [r["value"], r["fraction"]], equal_nan=True), (where, ps.value[i], ps.fraction[i], r["value"], r["fraction"])
        key = ms.match[i][r["mode"], r["conformer"]] if r["conformer"] >= 0 else np.full(len(ps.key[i]), -1)
        assert np.array_equal(ps.key[i], key), where
        assert ps.status[i] == ms.status[i], where
        chosen.append((int(ms.indices[i]), r["conformer"], key))
    # the chosen rows once more through the two calls: every output, bit for bit
    al_c = align(model, lib, [c[0] for c in chosen], [c[1] for c in chosen], [c[2] for c in chosen], weights=weights)
    rep_c = clashes(pocket, library=lib, indices=al_c.indices, conformers=al_c.conformers, rotation=al_c.rotation, translation=al_c.translation, node_radius=node_radius,
                    tolerance=tolerance, contact=contact)
    assert same_poses(ps.alignment(), al_c), tag
    assert same_report(ps.report(), rep_c), tag
    # ... and they are the bits the slot had in the call over all slots
    at = [i * M * stride + r["mode"] * stride + r["conformer"] for i, r in enumerate(rules) if r["conformer"] >= 0]
    have = [i for i, r in enumerate(rules) if r["conformer"] >= 0]
    assert np.array_equal(ps.alignment().rotation[have], al.rotation[at]) and np.array_equal(ps.alignment().translation[have], al.translation[at]), tag
    assert np.array_equal(ps.report().overlap[have], rep.overlap[at]) and np.array_equal(ps.report().n_clashing[have], rep.n_clashing[at]), tag
    return rules


def summary(tag, ps):
    chosen = ps.conformer >= 0
    print(f"{tag}: {len(ps)} hits, {int(chosen.sum())} posed, {int(ps.passes.sum())} pass, chosen away from (best conformer, mode 0): "
          f"{int((chosen & (ps.fraction < 1.0)).sum())}, candidates {int(ps.n_candidates.sum())}, dropped {int(ps.n_dropped.sum())}")


# ---------------------------------------------------------------------------------------------------------------- 1. the composition
CASES = (
    ("set_6oim_c8", 1, {}),
    ("set_6oim_c8", 4, {}),
    ("set_6oim_c8", 8, dict(max_clashing=1, min_fitted=3, min_fraction=0.9)),
    ("set_6oim_c8_weights", 4, {}),
    ("set_c21_c8", 4, {}),
    ("set_6oim_c1", 8, {}),  # conf_stride 1
    ("set_6oim_c64", 1, {}),  # 64 slots a hit: one full trip
    ("set_6oim_c64", 8, dict(min_fraction=0.5)),  # 512 slots a hit: eight trips
)


@pytest.mark.parametrize("name,modes,kw", CASES, ids=[f"{c[0]}-m{c[1]}" + ("-args" if c[2] else "") for c in CASES])
def test_equals_the_composition_bit_for_bit(name, modes, kw):
    from pharmaconet_amd.engine import explain_modes, pose_search

    model, lib, weights, d = load_golden(name)
    pocket = pocket_6oim()
    idx = small_trees(d, 12 if "c64" in name else 24)
    stride = int(lib.headers()[idx, 1].max())
    assert stride == {"set_6oim_c1": 1, "set_6oim_c64": 64}.get(name, 8)
    ms = explain_modes(model, lib, idx, modes=modes, weights=weights)
    ps = pose_search(model, lib, pocket, idx, modes=modes, weights=weights, **kw)
    rules = composition(ms, ps, model, lib, pocket, weights, stride, tag=f"{name}, {modes} modes", **kw)
    summary(f"{name}, {modes} modes {kw}", ps)
    assert (ps.conformer >= 0).sum() > 0 and sum(r["n_candidates"] for r in rules) >= len(idx)
    if kw.get("min_fraction"):
        assert ps.n_dropped.sum() > 0 and (ps.fraction[ps.conformer >= 0] >= kw["min_fraction"] * (1 - 4 * EPS)).all()
    # from the modes a caller already holds: the same answer
    held = ms.pose_search(model, lib, pocket, weights=weights, **kw)
    for f in dataclasses.fields(ps):
        a, b = getattr(ps, f.name), getattr(held, f.name)
        if f.name == "poses":
            assert same_poses(a, b)
        elif f.name == "clash":
            from test_gpu_clash import same_bits as same_report

            assert same_report(a, b)
        elif f.name == "key":
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
        else:
            assert np.array_equal(a, b, equal_nan=True), f.name


# ---------------------------------------------------------------------------------------------------------------- 2. trip edges
def hand_made(model, lib, lig, modes, C, winners, tie=None):
    """A `ModeSet` of len(winners) hits, all library ligand `lig`: every slot (m, c < C) holds a positive value of its own and the key that
    puts every level on its first candidate (`pmx_align` takes any candidate key); the slot winners[h] = m * C + c of hit h holds the
    largest. `tie`: (hit, slot): a second slot of that hit with the winner's value."""
    from pharmaconet_amd.engine import ModeSet

    rec = lib.unpack(lig)
    levels = np.asarray(ligand_levels(model, rec), dtype=np.int64)
    assert len(levels) >= 2
    first = np.array([candidates(model, rec, int(q))[0] for q in levels], dtype=np.int64)
    full = rec["n_conf"]
    values, match = [], []
    for h, win in enumerate(winners):
        v = np.zeros((modes, full))
        v[:, :C] = 1.0 + np.random.default_rng(100 + h).permutation(modes * C).reshape(modes, C) / 1024.0  # distinct, all below 2
        v[win // C, win % C] = 3.0
        if tie is not None and tie[0] == h:
            v[tie[1] // C, tie[1] % C] = 3.0
        values.append(v)
        match.append(np.broadcast_to(first, (modes, full, len(levels))).copy())
    n = len(winners)
    return ModeSet(indices=np.full(n, lig, np.int64), modes=modes, values=values, match=match, levels=[levels] * n, best_conformer=np.zeros(n, np.int64),
                   status=np.zeros(n, np.int32))


@pytest.mark.parametrize("modes,C", [(1, 1), (1, 63), (7, 9), (1, 64), (8, 8), (5, 13), (2, 64), (8, 16), (8, 64)], ids=lambda v: str(v))
def test_trip_edges(modes, C):
    """Slots per hit 1, 63, 64, 65 (13 conformers x 5 modes), 128 and 512: with every clash allowed each candidate passes and the choice is the
    largest value, which the test places first, last and on each side of every trip edge; with none allowed the overlaps decide. Both
    against the composition."""
    model, lib, weights, _ = load_golden("set_6oim_c64")
    pocket = pocket_6oim()
    lig = int(np.flatnonzero(lib.headers()[:, 1] == 64)[0])
    S = modes * C
    winners = sorted({s for e in range(0, S + 1, 64) for s in (e - 1, e, e + 1) if 0 <= s < S} | {0, S - 1})
    ms = hand_made(model, lib, lig, modes, C, winners)
    ps = ms.pose_search(model, lib, pocket, weights=weights, max_clashing=64, conformers=C)
    composition(ms, ps, model, lib, pocket, weights, C, max_clashing=64, tag=f"{modes} x {C}")
    assert (ps.n_candidates == S).all() and (ps.n_passing == S).all() and ps.passes.all()
    assert (ps.mode * C + ps.conformer).tolist() == winners and (ps.value == 3.0).all() and (ps.fraction == 1.0).all()
    # two slots with the winner's value: the lower conformer, then the lower mode - wherever the two stand in the trips
    if S > 1:
        for a, b in {(0, S - 1), (S - 1, 0), (min(63, S - 2), min(64, S - 1)), (S // 2, S // 2 - 1)}:
            tied = hand_made(model, lib, lig, modes, C, [a], tie=(0, b))
            got = tied.pose_search(model, lib, pocket, weights=weights, max_clashing=64, conformers=C)
            want = min((a, b), key=lambda s: (s % C, s // C))
            assert (int(got.conformer[0]), int(got.mode[0])) == (want % C, want // C), (a, b)
    strict = ms.pose_search(model, lib, pocket, weights=weights, conformers=C)
    rules = composition(ms, strict, model, lib, pocket, weights, C, tag=f"{modes} x {C}, strict")
    print(f"{modes} modes x {C} conformers = {S} slots, winners at {winners}; with no clash allowed: {rules[0]['n_passing']} of {S} slots pass")


# ---------------------------------------------------------------------------------------------------------------- 3. ragged and degenerate hits
def test_ragged_and_degenerate_hits_in_one_call():
    from pharmaconet_amd import PackedLibrary
    from pharmaconet_amd.engine import explain_modes, pose_search
    from pharmaconet_amd.library import UNSUPPORTED_RECORD, LigandFeatures, pack_ligand

    model, lib8, weights, d8 = load_golden("set_6oim_c8")
    _, lib1, _, _ = load_golden("set_6oim_c1")
    pocket = pocket_6oim()
    # a copy of a scoring ligand whose conformer 1 has conformer 0's coordinates
    small = small_trees(d8, 24)
    ms8 = explain_modes(model, lib8, small, modes=1, weights=weights)
    src = int(next(small[i] for i in range(24) if ms8.status[i] == 0 and ms8.values[i][0, 0] > 0 and small[i] + 1 in small))
    raw = np.frombuffer(lib8.record(src), dtype=np.uint8).copy()
    n, C, k = lib8.header(src)
    off = 8 + n + k
    off += -off % 4
    xyz = raw[off : off + 12 * n * C].view(np.float32).reshape(n, 3, C)
    xyz[:, :, 1] = xyz[:, :, 0]
    zero = pack_ligand(LigandFeatures([6, 8], [[1], [0]], [], np.zeros((2, 4, 3), np.float32)))  # no feature: it scores 0
    small = PackedLibrary.from_records([lib8.record(src), lib1.record(0), UNSUPPORTED_RECORD, zero, raw.tobytes(), lib8.record(src + 1)])
    idx = [0, 1, 2, 3, 4, 5, len(small) + 3, 0]  # conf_stride 8 above the second ligand's C = 1; outside the library; a duplicate
    ms = explain_modes(model, small, idx, modes=4, weights=weights)
    assert ms.status.tolist() == [0, 0, 1, 0, 0, 0, 1, 0] and ms.values[1].shape == (4, 1)
    ps = pose_search(model, small, pocket, idx, modes=4, weights=weights)
    composition(ms, ps, model, small, pocket, weights, 8, tag="ragged")
    assert ps.status.tolist() == ms.status.tolist()
    al, rep = ps.alignment(), ps.report()
    for i in (2, 3, 6):  # nothing to pose
        assert (ps.conformer[i], ps.mode[i], ps.passes[i], ps.n_candidates[i], ps.n_passing[i], ps.n_dropped[i]) == (-1, -1, False, 0, 0, 0)
        assert np.isnan(ps.value[i]) and np.isnan(ps.fraction[i]) and np.isnan(al.rotation[i]).all() and np.isnan(al.translation[i]).all() and np.isnan(rep.overlap[i])
        assert (ps.key[i] == -1).all() and al.n_nodes[i] == 0 and rep.n_clashing[i] == 0
    assert al.status[[2, 6]].tolist() == [1, 1] and rep.status[[2, 6]].tolist() == [1, 1] and al.status[3] != 0 and rep.status[3] != 0
    assert (al.status[[0, 1, 4, 5, 7]] == 0).all() and (rep.status[[0, 1, 4, 5, 7]] == 0).all()
    assert ps.conformer[1] == 0 and ps.n_candidates[1] <= 4  # one conformer: at most its four modes
    # the duplicate: the same row twice
    for f in ("conformer", "mode", "passes", "n_candidates", "n_passing", "value", "fraction"):
        assert getattr(ps, f)[0] == getattr(ps, f)[7], f
    assert np.array_equal(al.rotation[0], al.rotation[7]) and np.array_equal(rep.point_penetration[0], rep.point_penetration[7]) and np.array_equal(ps.key[0], ps.key[7])
    # the twin conformers: the same values, the same poses - the tie goes to conformer 0
    assert np.array_equal(ms.values[4][:, 0], ms.values[4][:, 1]) and np.array_equal(ms.match[4][:, 0], ms.match[4][:, 1])
    assert ps.conformer[4] != 1
    twin = pose_search(model, small, pocket, [4], modes=4, weights=weights, conformers=2, max_clashing=64)
    assert (twin.conformer[0], twin.mode[0], twin.n_candidates[0]) == (0, 0, int((ms.values[4][:, :2] > 0).sum())) and twin.value[0] == ms.values[4][0, 1]
    # no hits at all
    none = pose_search(model, small, pocket, [], modes=4, weights=weights)
    assert len(none) == 0 and len(none.alignment()) == 0 and len(none.report()) == 0


# ---------------------------------------------------------------------------------------------------------------- 4. the stated consequence
@pytest.mark.parametrize("name", ["set_6oim_c8", "set_6oim_c64"])
def test_a_default_pose_that_passes_is_the_choice(name):
    from pharmaconet_amd.engine import explain, pose_search
    from test_gpu_clash import same_bits as same_report

    model, lib, weights, d = load_golden(name)
    pocket = pocket_6oim()
    idx = small_trees(d, 32)
    ex = explain(model, lib, idx, weights=weights)
    al = ex.poses(model, lib, weights=weights)
    rep = al.clashes(pocket, lib)
    seen = 0
    for max_clashing in (0, 2):
        ps = pose_search(model, lib, pocket, idx, modes=4, weights=weights, max_clashing=max_clashing)
        ok = np.flatnonzero(rep.ok(max_clashing) & (al.status == 0) & (al.n_nodes >= 1))
        hits = al.rows[ok]
        assert np.array_equal(ps.conformer[hits], ex.best_conformer[hits]) and (ps.mode[hits] == 0).all() and ps.passes[hits].all() and (ps.fraction[hits] == 1.0).all()
        got, rg = ps.alignment(), ps.report()
        for r, h in zip(ok, hits):
            assert np.array_equal(got.rotation[h], al.rotation[r]) and np.array_equal(got.translation[h], al.translation[r]) and got.sse[h] == al.sse[r]
            assert np.array_equal(got.node[h], al.node[r]) and np.array_equal(ps.key[h], ex.match[h][ex.best_conformer[h]])
        assert same_report(dataclasses.replace(rg, **{f.name: ([getattr(rg, f.name)[h] for h in hits] if isinstance(getattr(rg, f.name), list) else getattr(rg, f.name)[hits])
                                                      for f in dataclasses.fields(rg) if f.name != "device"}), rep, rows=ok)
        print(f"{name}, max_clashing {max_clashing}: the default pose passes for {len(ok)} of {len(al)} hits, the search poses {int(ps.passes.sum())}")
        seen += len(ok)
    assert seen > 0


# ---------------------------------------------------------------------------------------------------------------- 5. the NumPy chain
def test_against_the_numpy_chain_on_the_fixture():
    """The 13 ligands of modes_set_6oim_c8 through align_ref, clash_ref and the rule, on the modes the GPU found (its totals are the product
    walker's float64 sums and agree with the fixture's, the reference's, to 2e-6 only - tests/test_gpu_modes.py - so the fixture's own
    totals would put a rounding error into a rule that compares bits). The chain's margins are asserted here as
    tests/test_pose_search_cpu.py asserts them for the fixture's modes; then choices and integers must be equal. The restatement's fit is
    NumPy's and the GPU's is its own, 1e-8 A apart in a posed coordinate where the rotation is unique (tests/test_gpu_align.py): a
    penetration, a difference of distances between such points, may differ by sqrt(3) * 1e-8 A. At the GPU's own motion the bars are
    those of tests/test_gpu_clash.py. Where the rotation is not unique - every conformer of ligand 15 under its mode 0, one matched cluster
    whose nodes share a target - the two fits are both right and pose differently, so there the chain checks the GPU's motion."""
    import clash_ref
    from pharmaconet_amd.constants import weights_vector
    import align_ref
    from explain_ref import Tables
    from pharmaconet_amd.engine import align, explain_modes, pose_search
    from test_gpu_clash import close
    from test_pose_search_cpu import fixture_chain

    model, lib, weights, _ = load_golden("set_6oim_c8")
    w7 = weights_vector(weights)
    pocket = pocket_6oim()
    fixture = fixture_chain()
    idx = [h["index"] for h in fixture]
    ms = explain_modes(model, lib, idx, modes=4, weights=weights)
    assert (ms.status == 0).all() and all(ms.best_conformer[i] == h["best"] for i, h in enumerate(fixture))
    Y = float(np.abs(model.node_centers).max())
    worst = np.zeros(2)
    # every slot's row through the restatements once; where the restatement's rotation is not unique (`pose_search_ref.unique`) the clash
    # check is made at the motion `align` gives that slot - no hit and no slot is left out
    slots = [(i, m, c) for i in range(len(idx)) for m in range(4) for c in range(8) if ms.values[i][m, c] > 0]
    al_all = align(model, lib, [idx[i] for i, _, _ in slots], [c for _, _, c in slots], [ms.match[i][m, c] for i, m, c in slots], weights=weights)
    caches, loose = [{} for _ in idx], 0
    Yc = align_ref.node_centers(model)
    tables = [Tables(model, lib.unpack(lig), w7) for lig in idx]
    for row, (i, m, c) in enumerate(slots):
        rec = lib.unpack(idx[i])
        s = psr.slot(model, rec, w7, pocket, ms.levels[i], ms.match[i][m, c], c, tables[i], Yc)
        if s["align_ok"] and not psr.unique(s["fit"]):
            loose += 1
            s = psr.slot(model, rec, w7, pocket, ms.levels[i], ms.match[i][m, c], c, tables[i], Yc, motion=(al_all.rotation[row], al_all.translation[row]))
        caches[i][m, c] = s
    print(f"{len(slots)} slots, {loose} of them with a rotation that is not unique (checked at the GPU's motion)")
    for modes in (1, 4):
        ps = pose_search(model, lib, pocket, idx, modes=modes, weights=weights)
        al, rep = ps.alignment(), ps.report()
        margin = np.inf
        for i, lig in enumerate(idx):
            rec = lib.unpack(lig)
            ref = psr.chain(model, rec, w7, pocket, ms.levels[i], ms.values[i], ms.match[i], modes, 8, cache=caches[i])
            margin = min([margin] + [s["margin"] for s in ref["rows"].values()])
            where = (modes, lig)
            got = (int(ps.conformer[i]), int(ps.mode[i]), bool(ps.passes[i]), int(ps.n_candidates[i]), int(ps.n_passing[i]), int(ps.n_dropped[i]))
            print(f"{modes} modes, ligand {lig}: GPU {got}, chain {(ref['conformer'], ref['mode'], ref['passes'], ref['n_candidates'], ref['n_passing'], ref['n_dropped'])}")
            assert got == (ref["conformer"], ref["mode"], ref["passes"], ref["n_candidates"], ref["n_passing"], ref["n_dropped"]), (where, got)
            assert ps.value[i] == ref["value"] and ps.fraction[i] == ref["fraction"], where
            row = ref["rows"][ref["mode"], ref["conformer"]]
            fit, cl = row["fit"], row["clash"]
            assert (int(al.n_nodes[i]), int(al.n_pairs[i])) == (fit["n_nodes"], fit["n_pairs"]) and al.status[i] == 0 and rep.status[i] == 0, where
            got_counts = [rep.n_points[i], rep.n_clashing[i], rep.n_pairs[i], rep.n_contacts[i], rep.worst[i, 0], rep.worst[i, 1]]
            assert [int(v) for v in got_counts] == cl["counts"].tolist(), where
            assert np.array_equal(rep.point_atom[i], cl["point_atom"]) and np.array_equal(rep.contact_fingerprint[i], cl["fingerprint"]), where
            A = max(Y, float(np.abs(rec["xyz"]).max()))
            bar = 1e-10 * fit["E0"] + fit["W"] * (16 * EPS * A) ** 2  # tests/test_gpu_align.py
            worst[0] = max(worst[0], abs(al.sse[i] - fit["sse"]) / bar)
            assert abs(al.sse[i] - fit["sse"]) <= bar, (where, al.sse[i], fit["sse"])
            if psr.unique(fit):
                dp = float(np.abs(rep.point_penetration[i] - cl["point_pen"]).max())
                worst[1] = max(worst[1], dp)
                assert dp <= np.sqrt(3.0) * 1e-8, (where, dp)
            # at the GPU's own motion
            nodes = rec["xyz"][:, :, int(ps.conformer[i])].astype(np.float32)
            r = clash_ref.clash_row(pocket.xyz, pocket.radius, pocket.group, nodes, np.float32(1.0), al.rotation[i], al.translation[i])
            assert r["margin"] >= 1e-9 and [int(v) for v in got_counts] == r["counts"].tolist(), where
            assert close(rep.point_penetration[i], r["point_pen"], 1e-12) and close(rep.clearance[i], r["clearance"], 1e-12), where
            assert abs(rep.overlap[i] - r["overlap"]) <= 1e-10 * r["overlap"], where
        print(f"{modes} modes: {int(ps.passes.sum())} of {len(idx)} hits have a passing pose; smallest clash margin of the chain {margin:.3g} (bar 1e-9)")
        assert margin >= 1e-9
        assert int(ps.passes.sum()) == {1: 4, 4: 7}[modes] == sum(h["one" if modes == 1 else "four"]["passes"] for h in fixture)
    print(f"against the NumPy chain: sse {worst[0]:.3g} of its bar, penetrations within {worst[1]:.3g} A (bar 1.73e-8)")


# ---------------------------------------------------------------------------------------------------------------- 6. the Python layer
def test_alignment_report_and_the_one_ligand_form():
    from pharmaconet_amd.engine import pose_search
    from test_attribution_cpu import load_mols
    from test_gpu_clash import same_bits as same_report

    model, lib, weights, d = load_golden("set_6oim_c8")
    pocket = pocket_6oim()
    idx = small_trees(d, 16)
    ps = pose_search(model, lib, pocket, idx, modes=4, weights=weights)
    again = pose_search(model, lib, pocket, idx, modes=4, weights=weights)
    for f in ("conformer", "mode", "passes", "n_candidates", "n_passing", "n_dropped", "value", "fraction", "status"):
        assert np.array_equal(getattr(ps, f), getattr(again, f), equal_nan=True), f
    assert same_poses(ps.alignment(), again.alignment()) and same_report(ps.report(), again.report())  # two runs, the same bits
    assert same_report(ps.alignment().clashes(pocket, lib), ps.report())
    perm = np.random.default_rng(5).permutation(16)
    moved = pose_search(model, lib, pocket, idx[perm], modes=4, weights=weights)
    assert np.array_equal(moved.conformer, ps.conformer[perm]) and np.array_equal(moved.alignment().rotation, ps.alignment().rotation[perm], equal_nan=True)
    assert same_report(moved.report(), ps.report(), rows=perm)  # ... and wherever the hit stands in the call
    # the chosen poses at atom level, and refined, through the ordinary Alignment
    mols = load_mols("set_6oim_c8")
    posed = np.flatnonzero(ps.conformer >= 0)
    atoms = ps.alignment().clashes(pocket, atoms=[mols[int(i)] for i in idx])
    assert len(atoms) == 16 and (atoms.status[posed] == 0).all() and (atoms.n_points[posed] > ps.report().n_points[posed]).any()
    ref = ps.alignment().refine(pocket, lib)
    assert (ref.status[posed] == 0).all() and np.array_equal(ref.overlap_start[posed], ps.report().overlap[posed])
    # one ligand
    r = int(posed[0])
    i = int(idx[r])
    one = model.scoring_pose_search(mols[i], modes=4, weights=weights, pocket=pocket)
    assert (one["conformer"], one["mode"], one["passes"], one["n_candidates"]) == (ps.conformer[r], ps.mode[r], ps.passes[r], ps.n_candidates[r])
    assert np.array_equal(one["rotation"], ps.alignment().rotation[r]) and one["value"] == ps.value[r] and one["overlap"] == ps.report().overlap[r]
    want = ps.alignment().transform(r, np.asarray(mols[i].atom_positions, dtype=np.float64)[:, int(ps.conformer[r])])
    assert np.array_equal(one["positions"], want) and one["node_positions"].shape == (lib.header(i)[0], 3)
    packed = model.scoring_pose_search(lib.record(i), modes=4, weights=weights, pocket=pocket)
    assert packed["positions"] is None and np.array_equal(packed["node_positions"], one["node_positions"])
    with pytest.raises(ValueError):
        pose_search(model, lib, pocket, idx, modes=4, weights=weights, min_fraction=1.5)
    with pytest.raises(Exception):
        pose_search(model, lib, pocket, idx, modes=9, weights=weights)


def test_many_hits_are_chunked_with_one_answer():
    """8200 hits x 4 modes x 8 conformers is more than one call takes (65536 slots): the chunks' answers are those of the hits alone."""
    from pharmaconet_amd.engine import _search_chunks, pose_search

    model, lib, weights, d = load_golden("set_6oim_c8")
    pocket = pocket_6oim()
    base = small_trees(d, 20, cap=5000)
    idx = np.resize(base, 2100)
    chunks = list(_search_chunks(np.full(2100, 8), 4))
    assert chunks == [(0, 2048, 8), (2048, 2100, 8)] and list(_search_chunks(np.array([1, 64, 1]), 8)) == [(0, 3, 64)]
    assert list(_search_chunks(np.array([64] * 129), 8)) == [(0, 128, 64), (128, 129, 64)] and list(_search_chunks(np.zeros(0, np.int64), 4)) == []
    few = pose_search(model, lib, pocket, base, modes=4, weights=weights)
    many = pose_search(model, lib, pocket, idx, modes=4, weights=weights)
    rows = np.resize(np.arange(20), 2100)
    for f in ("conformer", "mode", "passes", "n_candidates", "n_passing", "value", "fraction", "status"):
        assert np.array_equal(getattr(many, f), getattr(few, f)[rows], equal_nan=True), f
    assert np.array_equal(many.alignment().rotation, few.alignment().rotation[rows], equal_nan=True)
    assert np.array_equal(many.report().overlap, few.report().overlap[rows], equal_nan=True) and np.array_equal(many.report().status, few.report().status[rows])


def test_fitting_with_the_search():
    from test_gpu_clash import same_bits as same_report

    model, lib, weights, d = load_golden("set_6oim_c8")
    pocket = pocket_6oim()
    sel = small_trees(d, 24)
    lib = lib.select(sel)
    res = model.screen(lib, weights=weights)
    plain = res.fitting(16, pool=16, pocket=pocket)
    off = res.fitting(16, pool=16, pocket=pocket, search=0)
    for f in dataclasses.fields(plain):  # search=0 is today's result, field for field
        a, b = getattr(plain, f.name), getattr(off, f.name)
        if f.name == "report":
            assert same_report(a, b)
        elif f.name == "poses":
            assert same_poses(a, b) and np.array_equal(a.rows, b.rows)
        elif f.name == "refined":
            assert a is None and b is None
        else:
            assert np.array_equal(a, b), f.name
    fit = res.fitting(16, pool=16, pocket=pocket, search=4)
    print(f"fitting(16, pool=16): {len(plain)} of 16 pass; with search=4: {len(fit)}")
    assert len(fit) >= len(plain) and set(plain.indices.tolist()) <= set(fit.indices.tolist())
    assert np.array_equal(fit.pool, plain.pool) and (np.diff(fit.ranks) > 0).all() and np.array_equal(fit.pool[fit.ranks], fit.indices)
    passes = fit.report.ok(0) & (fit.poses.status == 0)
    assert np.array_equal(fit.rows, np.flatnonzero(passes)[:16]) and np.array_equal(fit.scores, _scores(res, fit))
    assert same_report(fit.poses.clashes(pocket, lib), fit.report)
    narrow = res.fitting(16, pool=16, pocket=pocket, search=4, min_fraction=0.99, min_fitted=3)
    assert len(narrow) <= len(fit)
    both = res.fitting(16, pool=16, pocket=pocket, search=4, refine=True, refine_tolerance=0.0)
    print(f"with search=4 and the refinement at tolerance 0: {len(both)}")
    assert len(both) >= len(fit) and set(fit.rows.tolist()) <= set(both.rows.tolist())
    if both.refined is not None:  # the rows the search could not make pass were refined from the search's choice
        failing = ~fit.report.ok(0) & (fit.poses.status == 0)
        assert np.array_equal(both.poses.conformers, fit.poses.conformers) and np.array_equal(both.poses.rotation[~failing], fit.poses.rotation[~failing], equal_nan=True)
        start = fit.poses.refine(pocket, lib, tolerance=0.0)
        assert np.array_equal(both.refined.rotation, start.rotation, equal_nan=True) and np.array_equal(both.refined.overlap_start, start.overlap_start, equal_nan=True)
    mols = {}
    from test_attribution_cpu import load_mols

    all_mols = load_mols("set_6oim_c8")
    at_atoms = res.fitting(16, pool=16, pocket=pocket, search=4, atoms=lambda i: mols.setdefault(i, all_mols[int(sel[i])]))
    assert np.array_equal(at_atoms.poses.rotation, fit.poses.rotation, equal_nan=True) and (at_atoms.report.n_points > fit.report.n_points).any()


def _scores(res, fit):
    """The explained scores of the passing hits: what `fitting` without the search reports for the same ligands."""
    from pharmaconet_amd.engine import explain

    return explain(res.model, res.library, fit.indices, weights=res.weights).scores


def test_cli_pose_search_csv(tmp_path):
    from pharmaconet_amd.engine import pose_search
    from pharmaconet_amd.screening import POSE_SEARCH_HEADER, main

    model, lib, _, d = load_golden("set_6oim_c8")
    lib = lib.select(small_trees(d, 16))  # (a screen of 16 ligands: the command line is what is tested)
    libfile = tmp_path / "lib.pmxlib"
    lib.save(libfile)
    args = ["-p", str(GOLDEN / "model_6oim_like.pm"), "-d", str(libfile), "--explain", "5"]
    main(args + ["-o", str(tmp_path / "plain.csv"), "--explain_out", str(tmp_path / "plain_hits.csv"), "--poses", str(tmp_path / "plain_poses.csv")])
    main(args + ["-o", str(tmp_path / "with.csv"), "--explain_out", str(tmp_path / "hits.csv"), "--poses", str(tmp_path / "poses.csv"), "--pose_search", str(tmp_path / "search.csv"),
                 "--pose_search_modes", "4", "--protein", str(GOLDEN / "pocket_6oim.pdb"), "--clash_tolerance", "0.5"])
    for a, b in (("plain.csv", "with.csv"), ("plain_hits.csv", "hits.csv"), ("plain_poses.csv", "poses.csv")):
        assert (tmp_path / a).read_bytes() == (tmp_path / b).read_bytes()
    rows = (tmp_path / "search.csv").read_text().splitlines()
    poses = (tmp_path / "poses.csv").read_text().splitlines()
    assert rows[0] == POSE_SEARCH_HEADER == ("rank,path,conformer,mode,passes,candidates,passing,mode_score,fraction_of_best,clashing,overlap,clearance,rmsd,rmsd_nodes,fitted_nodes,"
                                             "r00,r01,r02,r10,r11,r12,r20,r21,r22,tx,ty,tz")
    assert len(rows) == len(poses) == 6 and all(len(r.split(",")) == 27 for r in rows)
    assert [r.split(",")[:2] for r in rows[1:]] == [r.split(",")[:2] for r in poses[1:]]
    order = [int(r.split(",")[1].rsplit("#", 1)[1]) for r in rows[1:]]
    ps = pose_search(model, lib, pocket_6oim(), order, modes=4)
    for r, row in enumerate(rows[1:]):
        cells = row.split(",")
        assert [int(cells[2]), int(cells[3]), int(cells[4]), int(cells[5]), int(cells[6])] == [ps.conformer[r], ps.mode[r], int(ps.passes[r]), ps.n_candidates[r], ps.n_passing[r]]
        assert cells[7] == repr(float(ps.value[r])) and cells[15] == repr(float(ps.alignment().rotation[r, 0, 0])) and cells[10] == repr(float(ps.report().overlap[r]))
    with pytest.raises(SystemExit):
        main(["-p", str(GOLDEN / "model_6oim_like.pm"), "-d", str(libfile), "-o", str(tmp_path / "x.csv"), "--pose_search", str(tmp_path / "s.csv")])
