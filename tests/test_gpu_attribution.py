"""`pmx_attribute` on the GPU (csrc/pmx_rows.hip): entries, node shares and totals of listed leaves, checked against the reference's
recorded numbers (tests/golden/attribution_<set>.npz), against `pmx_explain`'s maxima, against the NumPy restatement of
tests/attribution_ref.py, and for what it does with keys that are no leaf of the tree."""

from functools import lru_cache

import numpy as np
import pytest

from attribution_ref import attribution, prefilter_margin
from conftest import GOLDEN, load_golden
from explain_ref import NONE, Tables, candidates, first_max_key, tree_leaves

pytestmark = pytest.mark.gpu

SETS = ("set_6oim_c1", "set_6oim_c8", "set_6oim_c64", "set_c21_c8", "set_l110_c8", "set_s64_c8", "set_6oim_c8_weights")
REFERENCE_SETS = tuple(s for s in SETS if s != "set_l110_c8")
BAR = 2e-6  # of the leaf's total: the project's bar for a leaf total against a conformer maximum (test_gpu_explain.py)


@lru_cache(maxsize=None)
def explained(name):
    """A set, its explanation and the attribution of every OK ligand at its best conformer: computed once, shared, never written to."""
    from pharmaconet_amd.engine import explain

    model, lib, weights, d = load_golden(name)
    ex = explain(model, lib, np.arange(len(lib)), weights=weights)
    at = ex.attribution(model, lib, weights=weights)
    return model, lib, weights, d, ex, at


def upper_sum(entry):
    return float(np.triu(entry.astype(np.float64)).sum())


@pytest.mark.parametrize("name", REFERENCE_SETS)
def test_reference_attribution_fixtures(name):
    """The reference's own entries (matching_pair_scores_dict), per-node halves of its own terms and the leaf's score: within 2e-6 of the
    total (the reference sums in float32; a far-tail term's float32 z^2 rounding is relative to the term)."""
    from pharmaconet_amd.engine import attribute
    from test_attribution_cpu import attribution_rows

    model, lib, weights, _ = load_golden(name)
    rows = list(attribution_rows(np.load(GOLDEN / f"attribution_{name}.npz")))
    at = attribute(model, lib, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], weights=weights)
    worst = np.zeros(3)
    for r, (i, c, key, lv, entry, node, total) in enumerate(rows):
        assert at.status[r] == 0 and at.levels[r].tolist() == lv.tolist()
        k = len(at.node[r])
        dev = np.array([np.abs(at.entry[r] - entry).max(initial=0.0), np.abs(at.node[r] - node[:k]).max(initial=0.0), abs(at.total[r] - total)])
        worst = np.maximum(worst, dev / max(total, 1e-300))
        assert (dev <= BAR * total).all(), (name, i, dev, total)
        assert (node[k:] == 0).all()
    print(f"{name}: against the reference, of the total: entry {worst[0]:.3g} node {worst[1]:.3g} total {worst[2]:.3g}")


@pytest.mark.parametrize("name", SETS)
def test_attribution_of_explained_ligands(name):
    """Every OK ligand at its best conformer under its own key: valid, explain's levels, explain's maximum, and shares and entries that
    add up to the total. The sums are float64 sums of non-negative addends, so they differ from the total by at most (number of
    roundings) * spacing(total): with P <= n (n - 1) / 2 node pairs and E = nl (nl + 1) / 2 entries, 5 P + 2 E + n for the shares (per pair a
    product and an add in each of two nodes and an add in its entry's float64 sum; per entry a division and an add in the total; n adds of
    the shares) and 2 E for the entries."""
    model, lib, weights, d, ex, at = explained(name)
    assert len(at) == int((ex.status == 0).sum()) > 0
    for r, i in enumerate(at.rows):
        assert at.status[r] == 0, (name, i)
        assert at.indices[r] == ex.indices[i] and at.conformers[r] == ex.best_conformer[i]
        assert at.levels[r].tolist() == ex.levels[i].tolist()
        cm = float(ex.conf_max[i][ex.best_conformer[i]])
        tot = float(at.total[r])
        assert abs(tot - cm) <= BAR * cm, (name, i, tot, cm)
        n, nl = len(at.node[r]), len(at.levels[r])
        P, E = n * (n - 1) // 2, nl * (nl + 1) // 2
        assert (at.node[r] >= 0).all()
        assert abs(float(at.node[r].sum()) - tot) <= (5 * P + 2 * E + n) * np.spacing(tot), (name, i, at.node[r].sum(), tot)
        assert abs(upper_sum(at.entry[r]) - tot) <= 2 * E * np.spacing(tot), (name, i)
        assert (np.tril(at.entry[r], -1) == 0).all()
        rec = lib.unpack(int(at.indices[r]))
        for q in set(range(int(rec["n_clusters"]))) - {int(q) for q in at.levels[r]}:  # clusters outside the tree carry nothing
            assert (at.node[r][int(rec["cluster_end"][q - 1]) if q else 0 : int(rec["cluster_end"][q])] == 0).all()
    if name == "set_s64_c8":
        assert max(len(x) for x in at.node) == 64  # every lane owns a node


def test_level_cap():
    """22 single-node clusters that all have candidates (the fixture ligands stop at 14 clusters): 20 levels, and the nodes of the two
    clusters beyond them carry nothing."""
    from pharmaconet_amd import PackedLibrary
    from pharmaconet_amd.constants import weights_vector
    from pharmaconet_amd.engine import explain
    from pharmaconet_amd.library import LigandFeatures, pack_ligand

    model, _, weights, _ = load_golden("set_6oim_c8")
    rng = np.random.default_rng(11)
    pos = (np.asarray(model.flat.cluster_center).mean(axis=0) + rng.uniform(-5, 5, (22, 3, 3))).astype(np.float32)
    lib = rec = None
    for ftype in ("Halogen", "Cation", "Anion", "HBond_acceptor", "HBond_donor"):
        one = PackedLibrary.from_records([pack_ligand(LigandFeatures([9] * 22, [[] for _ in range(22)], [(ftype, a, a) for a in range(22)], pos))])
        if one.header(0)[2] == 22 and candidates(model, one.unpack(0), 0):
            lib, rec = one, one.unpack(0)
            break
    assert lib is not None
    ex = explain(model, lib, [0], weights=weights)
    at = ex.attribution(model, lib, weights=weights)
    assert at.status[0] == 0 and len(at.levels[0]) == 20 and len(at.node[0]) == 22
    assert (at.node[0][20:] == 0).all()
    w7 = weights_vector(weights)
    c = int(at.conformers[0])
    ref = attribution(model, rec, w7, ex.levels[0], ex.match[0][c], c)
    assert ref["valid"] and abs(at.total[0] - ref["total"]) <= BAR * ref["total"]
    assert np.abs(at.node[0] - ref["node"]).max() <= BAR * ref["total"] and np.array_equal(at.fails[0], ref["fails"])
    assert abs(at.total[0] - ex.conf_max[0][c]) <= BAR * ex.conf_max[0][c]


@pytest.mark.parametrize("name", SETS)
def test_against_the_restatement(name):
    """First 32 ligands (4 of the large model): every entry and every node share within 2e-6 of the restated total, fails exact."""
    from pharmaconet_amd.constants import weights_vector
    from pharmaconet_amd.engine import attribute

    model, lib, weights, d, ex, at = explained(name)
    w7 = weights_vector(weights)
    take = 4 if "l110" in name else 32
    cases = [(int(at.rows[r]), int(at.conformers[r]), ex.match[at.rows[r]][at.conformers[r]], at, r) for r in range(len(at)) if at.rows[r] < take]
    if name == "set_6oim_c64":  # conformer 63, not only the best one
        rows = [i for i in range(min(take, len(ex))) if ex.status[i] == 0 and len(ex.conf_max[i]) == 64]
        assert rows
        last = attribute(model, lib, ex.indices[rows], [63] * len(rows), [ex.match[i][63] for i in rows], weights=weights)
        cases += [(i, 63, ex.match[i][63], last, r) for r, i in enumerate(rows)]
    worst = np.zeros(3)
    tables = {}
    for i, c, key, got, r in cases:
        rec = lib.unpack(int(ex.indices[i]))
        T = tables.setdefault(i, Tables(model, rec, w7))
        ref = attribution(model, rec, w7, ex.levels[i], key, c, T)
        assert ref["valid"] and got.status[r] == 0, (name, i, c)
        tot = ref["total"]
        dev = np.array([np.abs(got.entry[r] - ref["entry"]).max(initial=0.0), np.abs(got.node[r] - ref["node"]).max(initial=0.0), abs(got.total[r] - tot)])
        worst = np.maximum(worst, dev / max(tot, 1e-300))
        assert (dev <= BAR * tot).all(), (name, i, c, dev, tot)
        assert np.array_equal(got.fails[r], ref["fails"]), (name, i, c)
    assert cases
    print(f"{name}: against the restatement, of the total: entry {worst[0]:.3g} node {worst[1]:.3g} total {worst[2]:.3g}")


@pytest.mark.parametrize("name", ("set_6oim_c8", "set_c21_c8"))
def test_other_leaves(name):
    """The 12 smallest trees: up to 8 leaves per ligand that are not the maximum of a conformer they hold, attributed at that conformer:
    valid, and the leaf's restated score."""
    from pharmaconet_amd.constants import weights_vector
    from pharmaconet_amd.engine import attribute

    model, lib, weights, d = load_golden(name)
    w7 = weights_vector(weights)
    idx = [int(i) for i in np.argsort(d["n_tree"], kind="stable") if d["n_tree"][i] <= 2000][:12]
    rows = []
    for i in idx:
        rec = lib.unpack(i)
        T = Tables(model, rec, w7)
        _, leaves = tree_leaves(model, rec, w7, T)
        best, keys = first_max_key(leaves, T.C)
        taken = 0
        for key, sc in leaves:
            c = next((c for c, v in sorted(sc.items()) if v < best[c] and tuple(key) != keys[c]), None)
            if c is not None and taken < 8:
                rows.append((i, c, np.asarray(key, dtype=np.int64), float(sc[c])))
                taken += 1
    assert rows
    at = attribute(model, lib, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], weights=weights)
    for r, (i, c, key, score) in enumerate(rows):
        assert at.status[r] == 0, (name, i, c, key)
        assert abs(at.total[r] - score) <= BAR * score, (name, i, c, at.total[r], score)


def test_invalid_keys():
    """Structural cases only: each is reported PMX_LIGAND_KEY_INVALID with NaN total and shares, and the rows around it stay what they are."""
    from pharmaconet_amd.constants import weights_vector
    from pharmaconet_amd.engine import attribute

    model, lib, weights, d, ex, base = explained("set_6oim_c8")
    w7 = weights_vector(weights)
    K = model.flat.num_clusters
    r0 = next(r for r in range(len(base)) if len(base.levels[r]) >= 2 and base.total[r] > 0)
    i0 = int(base.rows[r0])
    lig, c0 = int(ex.indices[i0]), int(base.conformers[r0])
    key0 = ex.match[i0][c0].copy()
    rec0 = lib.unpack(lig)
    cand0 = candidates(model, rec0, int(ex.levels[i0][0]))
    stranger = next(m for m in range(K) if m not in cand0)
    not_candidate, past_k = key0.copy(), key0.copy()
    not_candidate[0], past_k[0] = stranger, K
    # a pair of matches the cluster-distance prefilter rejects by more than 1 A for every conformer
    found = None
    for i in range(len(lib)):
        if ex.status[i] != 0 or found:
            continue
        rec = lib.unpack(i)
        T = Tables(model, rec, w7)
        lv = ex.levels[i]
        for l1 in range(len(lv)):
            for l2 in range(l1 + 1, len(lv)):
                for a1 in candidates(model, rec, int(lv[l1])):
                    for a2 in candidates(model, rec, int(lv[l2])):
                        if found is None and prefilter_margin(T, model, int(lv[l1]), a1, int(lv[l2]), a2) > 1.0:
                            found = (i, l1, a1, l2, a2)
    assert found is not None
    fi, l1, a1, l2, a2 = found
    far = np.full(len(ex.levels[fi]), NONE, dtype=np.int64)
    far[l1], far[l2] = a1, a2
    none = np.full(len(key0), NONE, dtype=np.int64)
    C0 = len(ex.conf_max[i0])
    rows = [(lig, c0, key0), (lig, c0, not_candidate), (lig, c0, past_k), (lig, C0, key0), (fi, 0, far), (len(lib), 0, none), (lig, c0, none), (lig, c0, key0)]
    at = attribute(model, lib, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], weights=weights)
    assert at.status.tolist() == [0, 4, 4, 4, 4, 1, 0, 0]
    for r in (1, 2, 3, 4, 5):
        assert np.isnan(at.total[r]) and np.isnan(at.node[r]).all()
    assert len(at.node[1]) == rec0["n_nodes"] and len(at.node[5]) == 0 and len(at.levels[5]) == 0
    assert at.entry[4][l1, l2] == -1.0 and at.entry[4][l1, l1] >= 0 and at.entry[4][l2, l2] >= 0
    assert (at.entry[3] == 0).all()  # (not a conformer of the ligand: nothing to compute)
    assert at.levels[1].tolist() == ex.levels[i0].tolist()
    assert at.total[6] == 0.0 and (at.node[6] == 0).all() and (at.entry[6] == 0).all()
    for r in (0, 7):
        assert at.total[r] == base.total[r0] and np.array_equal(at.node[r], base.node[r0])
        assert np.array_equal(at.entry[r], base.entry[r0]) and np.array_equal(at.fails[r], base.fails[r0])


def test_repeatable_and_leaves_the_stream_as_it_was():
    from pharmaconet_amd.engine import DeviceLibrary, attribute, explain, screen

    model, lib, weights, d, ex, base = explained("set_c21_c8")
    dlib = DeviceLibrary(lib)
    before = screen(model, dlib, weights=weights, float64=True).scores.cpu().numpy()
    rows = np.asarray(base.rows)
    keys = [ex.match[i][c] for i, c in zip(rows, base.conformers)]

    def same(a, ra, b, rb):
        return (np.array_equal(a.total[ra], b.total[rb], equal_nan=True) and np.array_equal(a.node[ra], b.node[rb], equal_nan=True)
                and np.array_equal(a.entry[ra], b.entry[rb]) and np.array_equal(a.fails[ra], b.fails[rb])
                and np.array_equal(a.levels[ra], b.levels[rb]) and a.status[ra] == b.status[rb])

    again = attribute(model, dlib, base.indices, base.conformers, keys, weights=weights)
    assert all(same(again, r, base, r) for r in range(len(base)))
    rep = np.concatenate([np.arange(len(base)), np.arange(len(base))[::-1], np.arange(min(3, len(base)))])
    twice = attribute(model, dlib, base.indices[rep], base.conformers[rep], [keys[r] for r in rep], weights=weights)
    assert all(same(twice, k, base, r) for k, r in enumerate(rep))
    empty = attribute(model, dlib, [], [], [], weights=weights)
    assert len(empty) == 0 and empty.total.size == 0
    after = screen(model, dlib, weights=weights, float64=True).scores.cpu().numpy()
    assert np.array_equal(before, after, equal_nan=True)
    ex2 = explain(model, dlib, ex.indices, weights=weights)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(ex2.conf_max, ex.conf_max))
    assert all(np.array_equal(a, b) for a, b in zip(ex2.match, ex.match))


def test_scoring_attribution_and_atom_scores():
    from test_attribution_cpu import load_mols

    model, lib, weights, d, ex, base = explained("set_6oim_c8")
    r = next(r for r in range(len(base)) if base.total[r] > 0)
    i = int(base.indices[r])
    det = model.scoring_attribution(lib.record(i), weights=weights)
    assert det["status"] == 0 and det["conformer"] == base.conformers[r] and det["total"] == base.total[r]
    assert np.array_equal(det["node"], base.node[r]) and np.array_equal(det["entry"], base.entry[r])
    sc = base.atom_scores(r, load_mols("set_6oim_c8")[i])
    assert abs(sc.sum() - base.total[r]) <= 4 * len(base.node[r]) * np.spacing(base.total[r])
    other = model.scoring_attribution(lib.record(i), weights=weights, conformer=0, key=np.full(len(det["levels"]), -1))
    assert other["status"] == 0 and other["total"] == 0.0


def test_cli_node_csv(tmp_path):
    from pharmaconet_amd.screening import main

    model, lib, _, _ = load_golden("set_6oim_c8")
    libfile = tmp_path / "lib.pmxlib"
    lib.save(libfile)
    args = ["-p", str(GOLDEN / "model_6oim_like.pm"), "-d", str(libfile)]
    main(args + ["-o", str(tmp_path / "plain.csv")])
    main(args + ["-o", str(tmp_path / "with.csv"), "--explain", "5", "--explain_out", str(tmp_path / "hits.csv"), "--explain_nodes", str(tmp_path / "nodes.csv")])
    assert (tmp_path / "plain.csv").read_bytes() == (tmp_path / "with.csv").read_bytes()
    hits = [row.split(",") for row in (tmp_path / "hits.csv").read_text().splitlines()[1:]]
    rows = (tmp_path / "nodes.csv").read_text().splitlines()
    assert rows[0] == "rank,index,path,conformer,node,node_types,ligand_cluster,model_cluster,node_score,share" and len(hits) == 5
    K = model.flat.num_clusters
    per_hit = {}
    for row in rows[1:]:
        f = row.split(",")
        assert len(f) == 10
        per_hit.setdefault(int(f[0]), []).append(f)
    assert sorted(per_hit) == [1, 2, 3, 4, 5]
    for rank, fs in per_hit.items():
        h = hits[rank - 1]
        i = int(fs[0][1])
        assert fs[0][2] == h[1] and int(fs[0][3]) == int(h[3])
        assert [int(f[4]) for f in fs] == list(range(lib.header(i)[0]))
        assert all(f[5] and 0 <= int(f[6]) < lib.header(i)[2] and (f[7] == "" or 0 <= int(f[7]) < K) for f in fs)
        cm = float(h[4])
        assert abs(sum(float(f[8]) for f in fs) - cm) <= BAR * cm
        assert abs(sum(float(f[9]) for f in fs) - 1.0) <= 1e-9
        assert all(float(f[8]) == 0 for f in fs if f[7] == "")
