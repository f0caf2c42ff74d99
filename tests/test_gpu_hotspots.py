"""`pmx_hotspots` on the GPU (csrc/pmx_rows.hip): model-node shares, term counts and interaction fingerprints of listed leaves, checked
against the NumPy restatement of tests/hotspot_ref.py, against `pmx_attribute` on the same rows, on a model of more than 192 nodes, for
what it does with keys that are no leaf of the tree, and through the Python and command-line front ends."""

from functools import lru_cache

import numpy as np
import pytest

from attribution_ref import prefilter_margin
from conftest import GOLDEN, load_golden
from explain_ref import NONE, Tables, candidates
from hotspot_ref import hotspots as restated
from hotspot_ref import words_to_bits
from test_gpu_attribution import BAR, SETS, explained

pytestmark = pytest.mark.gpu


@lru_cache(maxsize=None)
def profiled(name):
    """The hotspot profile of every OK ligand of a set at its best conformer, next to `explained(name)`: computed once, never written to."""
    model, lib, weights, d, ex, at = explained(name)
    return ex.hotspots(model, lib, weights=weights)


def cluster_members(model) -> np.ndarray:
    """bool [K, Nm]"""
    flat = model.flat
    cn = np.ascontiguousarray(np.asarray(flat.cluster_nodes, dtype=np.uint64).reshape(flat.num_clusters, -1))
    return np.unpackbits(cn.view(np.uint8), axis=1, bitorder="little")[:, : flat.num_nodes].astype(bool)


def check_against_restatement(model, lib, w7, ex, cases, what):
    """cases: (row of ex, conformer, key, profile, row of the profile). Shares within BAR of the restated total; counts and fingerprint exact."""
    worst, tables = 0.0, {}
    for i, c, key, got, r in cases:
        rec = lib.unpack(int(ex.indices[i]))
        T = tables.setdefault(i, Tables(model, rec, w7))
        ref = restated(model, rec, w7, ex.levels[i], key, c, T)
        assert ref["valid"] and got.status[r] == 0, (what, i, c)
        tot = ref["total"]
        dev = max(float(np.abs(got.share[r] - ref["share"]).max(initial=0.0)), abs(float(got.total[r]) - tot))
        worst = max(worst, dev / max(tot, 1e-300))
        assert dev <= BAR * tot, (what, i, c, dev, tot)
        assert np.array_equal(got.terms[r], ref["terms"]) and np.array_equal(got.passes[r], ref["passes"]), (what, i, c)
        assert np.array_equal(got.fingerprint[r], ref["fingerprint"]), (what, i, c)
        assert got.nodes(r).tolist() == np.flatnonzero((ref["terms"] > 0) & (2 * ref["passes"] >= ref["terms"])).tolist()
    assert cases
    print(f"{what}: against the restatement, of the total: {worst:.3g}")


@pytest.mark.parametrize("name", SETS)
def test_against_the_restatement(name):
    """The shapes of the attribution test of the same name: the first 32 ligands (4 of the 110-node model, whose nodes fill two node
    words) at their best conformer under its own key, and conformer 63 of the 64-conformer set."""
    from pharmaconet_amd.constants import weights_vector
    from pharmaconet_amd.engine import hotspots

    model, lib, weights, d, ex, at = explained(name)
    hs = profiled(name)
    take = 4 if "l110" in name else 32
    cases = [(int(hs.rows[r]), int(hs.conformers[r]), ex.match[hs.rows[r]][hs.conformers[r]], hs, r) for r in range(len(hs)) if hs.rows[r] < take]
    if name == "set_6oim_c64":
        rows = [i for i in range(min(take, len(ex))) if ex.status[i] == 0 and len(ex.conf_max[i]) == 64]
        assert rows
        last = hotspots(model, lib, ex.indices[rows], [63] * len(rows), [ex.match[i][63] for i in rows], weights=weights)
        cases += [(i, 63, ex.match[i][63], last, r) for r, i in enumerate(rows)]
    check_against_restatement(model, lib, weights_vector(weights), ex, cases, name)


@pytest.mark.parametrize("name", SETS)
def test_hotspots_of_explained_ligands(name):
    """Every OK ligand at its best conformer under its own key: total, levels and status are `pmx_attribute`'s bit for bit; the shares are
    not negative, vanish (with their fingerprint bits and counts) outside the model clusters the key matches, and add up to the total.

    The bound on |sum of the shares - total| counts float64 roundings of non-negative numbers that are at most the total, each worth at most
    spacing(total). With n ligand nodes, P <= n (n - 1) / 2 node pairs, E = nl (nl + 1) / 2 entries, S the largest model cluster (no node
    subset is larger) and Nm model nodes:
      S^2 + S + 1  relative error of one contribution coef * rowsum: S^2 - 1 adds in G, S - 1 adds in the row sum, the product term * scale,
                   the division by G and the product with the row sum (the factor 1/2 is exact)
      P + 1        scale[e]: the P - 1 adds of the entry's float64 sum of terms at most, and its division
      2 P          adds into one model node's sum: at most two contributions per node pair
      2 E          the total: every entry is added once, and once more per level the pair entries' partial sum
      Nm           the sum of the shares taken here"""
    model, lib, weights, d, ex, at = explained(name)
    hs = profiled(name)
    assert len(hs) == len(at) > 0 and np.array_equal(hs.rows, at.rows)
    assert np.array_equal(hs.total.view(np.uint64), at.total.view(np.uint64)) and np.array_equal(hs.status, at.status)
    assert np.array_equal(hs.indices, at.indices) and np.array_equal(hs.conformers, at.conformers)
    members = cluster_members(model)
    nm, S = model.flat.num_nodes, int(members.sum(axis=1).max())
    assert hs.fingerprint.shape == (len(hs), 4) and hs.fingerprint.dtype == np.uint64
    bits = words_to_bits(hs.fingerprint)
    assert not bits[:, nm:].any()
    engaged = 0
    for r, i in enumerate(hs.rows):
        assert hs.status[r] == 0 and hs.levels[r].tolist() == at.levels[r].tolist()
        tot = float(hs.total[r])
        n, nl = len(at.node[r]), len(at.levels[r])
        P, E = n * (n - 1) // 2, nl * (nl + 1) // 2
        share = hs.share[r]
        assert share.shape == (nm,) and (share >= 0).all(), (name, i)
        rounds = (S * S + S + 1) + (P + 1) + 2 * P + 2 * E + nm
        assert abs(float(share.sum()) - tot) <= rounds * np.spacing(tot), (name, i, share.sum(), tot)
        key = ex.match[i][hs.conformers[r]]
        inside = members[[int(k) for k in key if k != NONE]].any(axis=0) if (key != NONE).any() else np.zeros(nm, dtype=bool)
        assert (share[~inside] == 0).all() and (hs.terms[r][~inside] == 0).all() and not bits[r, :nm][~inside].any(), (name, i)
        assert (hs.passes[r] <= hs.terms[r]).all() and (share[hs.terms[r] == 0] == 0).all()
        assert np.array_equal(bits[r, :nm], (hs.terms[r] > 0) & (2 * hs.passes[r] >= hs.terms[r]))
        engaged += int(bits[r].sum())
    assert engaged > 0


def enlarged(model, copies: int):
    """`model` with every node `copies` times (node m + t * Nm is copy t of node m, its edges shifted by a few hundredths of an Angstrom
    per copy) and every cluster spread over the copies: member m of cluster a becomes its copy (m + a) % copies. Cluster sizes, types, centres
    and so the candidates stay what they are; the node indices fill all the node words."""
    from pharmaconet_amd import PharmacophoreModel
    from pharmaconet_amd.pharmacophore_model import FlatModel, _node_masks, cluster_node_sets

    flat = model.flat
    nm = flat.num_nodes
    t = np.repeat(np.arange(copies), nm)
    shift = (0.03 * ((t[:, None] + t[None, :]) % 4)).astype(np.float32)
    masks = []
    for a, mask in enumerate(cluster_node_sets(flat)):
        masks.append(sum(1 << (m + ((m + a) % copies) * nm) for m in range(nm) if (mask >> m) & 1))
    big = PharmacophoreModel()
    big._state = model._state
    big._flat = FlatModel(node_type=np.tile(flat.node_type, copies), edge_mean=np.ascontiguousarray(np.tile(flat.edge_mean, (copies, copies)) + shift),
                          edge_std=np.ascontiguousarray(np.tile(flat.edge_std, (copies, copies))), cluster_nodes=_node_masks(masks, nm * copies),
                          cluster_typemask=flat.cluster_typemask, cluster_center=flat.cluster_center, cluster_size=flat.cluster_size, cluster_type=flat.cluster_type)
    return big


def test_a_model_of_four_node_words():
    """222 model nodes (the 37-node fixture model six times): the members of a cluster lie in different node words, the last of them in
    word 3. Six ligands against the restatement."""
    from pharmaconet_amd.constants import weights_vector
    from pharmaconet_amd.engine import explain

    model, lib, weights, _ = load_golden("set_6oim_c8")
    big = enlarged(model, 6)
    assert 192 < big.flat.num_nodes <= 256
    ex = explain(big, lib, np.arange(12), weights=weights)
    hs = ex.hotspots(big, lib, weights=weights)
    rows = [r for r in range(len(hs)) if hs.total[r] > 0][:6]
    assert len(rows) >= 4
    cases = [(int(hs.rows[r]), int(hs.conformers[r]), ex.match[hs.rows[r]][hs.conformers[r]], hs, r) for r in rows]
    check_against_restatement(big, lib, weights_vector(weights), ex, cases, "222 nodes")
    assert any(hs.share[r][192:].sum() > 0 for r in rows) and any(hs.fingerprint[r, 3] != 0 for r in rows)
    assert all(len(hs.share[r]) == 222 for r in rows)


def test_invalid_rows():
    """A key that is no leaf (a pair of matches the cluster-distance prefilter rejects), a conformer the ligand does not have, a match that is
    no candidate of its level, an index outside the library: reported with NaN total and shares and zero counts and fingerprint, and the
    rows around them stay what they are. The all-None key is valid with everything zero; an empty call succeeds."""
    from pharmaconet_amd.constants import weights_vector
    from pharmaconet_amd.engine import hotspots

    model, lib, weights, d, ex, at = explained("set_6oim_c8")
    base = profiled("set_6oim_c8")
    w7 = weights_vector(weights)
    K, nm = model.flat.num_clusters, model.flat.num_nodes
    r0 = next(r for r in range(len(base)) if len(base.levels[r]) >= 2 and base.total[r] > 0)
    i0 = int(base.rows[r0])
    lig, c0 = int(ex.indices[i0]), int(base.conformers[r0])
    key0 = ex.match[i0][c0].copy()
    cand0 = candidates(model, lib.unpack(lig), int(ex.levels[i0][0]))
    not_candidate, past_k = key0.copy(), key0.copy()
    not_candidate[0], past_k[0] = next(m for m in range(K) if m not in cand0), K
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
    hs = hotspots(model, lib, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], weights=weights)
    assert hs.status.tolist() == [0, 4, 4, 4, 4, 1, 0, 0]
    for r in (1, 2, 3, 4, 5):
        assert np.isnan(hs.total[r]) and np.isnan(hs.share[r]).all() and len(hs.share[r]) == nm
        assert (hs.terms[r] == 0).all() and (hs.passes[r] == 0).all() and (hs.fingerprint[r] == 0).all()
    assert hs.levels[1].tolist() == ex.levels[i0].tolist() and len(hs.levels[5]) == 0
    assert hs.total[6] == 0.0 and (hs.share[6] == 0).all() and (hs.terms[6] == 0).all() and (hs.fingerprint[6] == 0).all()
    for r in (0, 7):
        assert hs.total[r] == base.total[r0] and np.array_equal(hs.share[r], base.share[r0]) and np.array_equal(hs.fingerprint[r], base.fingerprint[r0])
        assert np.array_equal(hs.terms[r], base.terms[r0]) and np.array_equal(hs.passes[r], base.passes[r0])
    empty = hotspots(model, lib, [], [], [], weights=weights)
    assert len(empty) == 0 and empty.total.size == 0 and empty.fingerprint.shape == (0, 4)


def test_repeatable_and_leaves_the_stream_as_it_was():
    from pharmaconet_amd.engine import DeviceLibrary, attribute, hotspots, screen

    model, lib, weights, d, ex, at = explained("set_c21_c8")
    base = profiled("set_c21_c8")
    dlib = DeviceLibrary(lib)
    before = screen(model, dlib, weights=weights, float64=True).scores.cpu().numpy()
    keys = [ex.match[i][c] for i, c in zip(base.rows, base.conformers)]

    def same(a, ra, b, rb):
        return (np.array_equal(a.total[ra], b.total[rb], equal_nan=True) and np.array_equal(a.share[ra], b.share[rb], equal_nan=True)
                and np.array_equal(a.terms[ra], b.terms[rb]) and np.array_equal(a.passes[ra], b.passes[rb])
                and np.array_equal(a.fingerprint[ra], b.fingerprint[rb]) and np.array_equal(a.levels[ra], b.levels[rb]) and a.status[ra] == b.status[rb])

    again = hotspots(model, dlib, base.indices, base.conformers, keys, weights=weights)
    assert all(same(again, r, base, r) for r in range(len(base)))
    rep = np.concatenate([np.arange(len(base)), np.arange(len(base))[::-1], np.arange(min(3, len(base)))])
    twice = hotspots(model, dlib, base.indices[rep], base.conformers[rep], [keys[r] for r in rep], weights=weights)
    assert all(same(twice, k, base, r) for k, r in enumerate(rep))
    after = screen(model, dlib, weights=weights, float64=True).scores.cpu().numpy()
    assert np.array_equal(before, after, equal_nan=True)
    at2 = attribute(model, dlib, at.indices, at.conformers, keys, weights=weights)  # (the kernel that shares its steps, after it)
    assert np.array_equal(at2.total, at.total) and all(np.array_equal(a, b) for a, b in zip(at2.node, at.node))


def test_front_ends():
    """`Explanation.hotspots` on a mode's explanation, `scoring_hotspots`, `usage`, `cluster_share` and `ScreeningResult.diverse`."""
    from pharmaconet_amd.engine import explain_modes, screen

    model, lib, weights, d, ex, at = explained("set_6oim_c8")
    base = profiled("set_6oim_c8")
    nm = model.flat.num_nodes
    r = next(r for r in range(len(base)) if base.total[r] > 0)
    i = int(base.indices[r])
    det = model.scoring_hotspots(lib.record(i), weights=weights)
    assert det["status"] == 0 and det["conformer"] == base.conformers[r] and det["total"] == base.total[r]
    assert np.array_equal(det["share"], base.share[r]) and np.array_equal(det["fingerprint"], base.fingerprint[r]) and det["nodes"].tolist() == base.nodes(r).tolist()
    other = model.scoring_hotspots(lib.record(i), weights=weights, conformer=0, key=np.full(len(det["levels"]), -1))
    assert other["status"] == 0 and other["total"] == 0.0 and len(other["nodes"]) == 0

    ms = explain_modes(model, lib, ex.indices[:8], modes=2, weights=weights)
    second = ms.explanation(1)
    hs1 = second.hotspots(model, lib, weights=weights)
    assert len(hs1) == int((ms.status == 0).sum()) and (hs1.status == 0).all()
    seen = 0
    for q, row in enumerate(hs1.rows):
        v = float(ms.values[row][1, hs1.conformers[q]])
        assert abs(hs1.total[q] - v) <= BAR * v
        seen += v > 0
    assert seen > 0

    use = base.usage()
    assert use.shape == (nm,) and (use >= 0).all() and abs(use.sum() - 1.0) <= 1e-9
    members = cluster_members(model)
    cs = base.cluster_share(r, model)
    assert cs.shape == (model.flat.num_clusters,)
    assert np.allclose(cs, [base.share[r][members[a]].sum() for a in range(len(members))], rtol=1e-12, atol=0)
    assert cs.sum() >= base.total[r] * (1 - 1e-12)  # (a node of several clusters counts in each)

    res = screen(model, lib, weights=weights)
    dv = res.diverse(5, pool=48, threshold=0.7)
    prof = dv.profile
    assert len(dv.pool) == len(prof) == len(dv.leader_of) == int((ex.status[res._best(48).astype(np.int64)] == 0).sum())
    assert 1 <= len(dv) <= 5 and dv.leaders[0] == 0 and (np.diff(dv.leaders) > 0).all()
    assigned = dv.leader_of >= 0
    assert (dv.leader_of[assigned] <= np.flatnonzero(assigned)).all() and np.isin(dv.leader_of[assigned], dv.leaders).all()
    assert (dv.leader_of[dv.leaders] == dv.leaders).all()
    sim = prof.similarity()
    assert sim.shape == (len(prof), len(prof)) and sim.dtype == np.float32
    lead = sim[np.ix_(dv.leaders, dv.leaders)]
    assert (lead[~np.eye(len(dv), dtype=bool)] < np.float32(0.7)).all()
    assert (sim[np.flatnonzero(assigned), dv.leader_of[assigned]] >= np.float32(0.7)).all()
    assert int(dv.cluster_size.sum()) == int(assigned.sum()) and (dv.cluster_size >= 1).all()
    assert np.array_equal(dv.indices, dv.pool[dv.leaders])
    scores = res.scores.cpu().numpy().astype(np.float64)
    assert np.allclose(dv.scores, scores[dv.indices], rtol=1e-5)
    lone, lone_of = prof.leaders(threshold=1.0)
    assert (lone_of >= 0).all() and len(lone) == len(np.unique(prof.fingerprint, axis=0))


def test_cli_hotspot_and_diverse_csv(tmp_path):
    from pharmaconet_amd.constants import TYPE_NAMES
    from pharmaconet_amd.screening import main

    model, lib, _, _ = load_golden("set_6oim_c8")
    libfile = tmp_path / "lib.pmxlib"
    lib.save(libfile)
    args = ["-p", str(GOLDEN / "model_6oim_like.pm"), "-d", str(libfile)]
    main(args + ["-o", str(tmp_path / "plain.csv")])
    main(args + ["-o", str(tmp_path / "with.csv"), "--explain", "5", "--explain_out", str(tmp_path / "hits.csv"), "--hotspots", str(tmp_path / "hot.csv"),
                 "--diverse", "3", "--diverse_pool", "24", "--diverse_threshold", "0.6", "--diverse_out", str(tmp_path / "div.csv")])
    assert (tmp_path / "plain.csv").read_bytes() == (tmp_path / "with.csv").read_bytes()
    hits = [row.split(",") for row in (tmp_path / "hits.csv").read_text().splitlines()[1:]]
    rows = (tmp_path / "hot.csv").read_text().splitlines()
    assert rows[0] == "rank,path,node,type,share,fraction,engaged" and len(hits) == 5
    per_hit = {}
    for row in rows[1:]:
        f = row.split(",")
        assert len(f) == 7
        per_hit.setdefault(int(f[0]), []).append(f)
    assert sorted(per_hit) == [1, 2, 3, 4, 5]
    for rank, fs in per_hit.items():
        h = hits[rank - 1]
        assert all(f[1] == h[1] for f in fs)
        nodes = [int(f[2]) for f in fs]
        assert nodes == sorted(set(nodes)) and all(0 <= m < model.flat.num_nodes for m in nodes)
        assert all(f[3] == TYPE_NAMES[int(model.flat.node_type[int(f[2])])] and f[6] in ("0", "1") for f in fs)
        cm = float(h[4])
        assert abs(sum(float(f[4]) for f in fs) - cm) <= BAR * cm
        assert abs(sum(float(f[5]) for f in fs) - 1.0) <= 1e-9
    main_rows = (tmp_path / "plain.csv").read_text().splitlines()[1:]
    div = (tmp_path / "div.csv").read_text().splitlines()
    assert div[0] == "rank,path,score,cluster_size,engaged_nodes" and 2 <= len(div) <= 4
    ranks = []
    for row in div[1:]:
        f = row.split(",")
        assert len(f) == 5 and main_rows[int(f[0]) - 1] == f"{f[1]},{f[2]}"  # (the main CSV's row of that rank)
        assert int(f[3]) >= 1 and all(0 <= int(m) < model.flat.num_nodes for m in f[4].split())
        ranks.append(int(f[0]))
    assert ranks[0] == 1 and ranks == sorted(set(ranks)) and sum(int(row.split(",")[3]) for row in div[1:]) <= 24
