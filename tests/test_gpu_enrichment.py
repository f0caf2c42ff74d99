"""pmx_enrichment on the GPU against the NumPy restatement of its specification (tests/enrichment_ref.py): integers exact, hits bit for
bit, expsum to 1e-11 relative - every term is positive, so a sum of G of them in any order plus a few ulp for exp / expm1 stays within
(G + 16) 2^-52, 1.8e-12 for the at most 8 200 groups used here."""

import re

import numpy as np
import pytest

import enrichment_ref as ref
from conftest import GOLDEN, REPO, load_golden

pytestmark = pytest.mark.gpu

EXPSUM_RTOL = 1e-11
CUT = (0.005, 0.01, 0.05, 1.0)  # the last one is 10^6 ppm: the whole list


def tile():
    from pharmaconet_amd import engine

    t = int(engine.ENRICH_TILE)
    assert t == int(re.search(r"#define PMX_ENRICH_TILE (\d+)", (REPO / "include" / "pmx.h").read_text()).group(1))
    return t


def run(scores, labels, status=None, cutoffs=CUT, alpha=20.0, bootstrap=0, seed=0, order=True):
    import torch

    from pharmaconet_amd import engine

    sc = scores if isinstance(scores, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32)).cuda()
    return engine.enrichment(sc, labels, status=status, cutoffs=cutoffs, alpha=alpha, bootstrap=bootstrap, seed=seed, order=order)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def expsum_deviation(got, want):
    with np.errstate(divide="ignore", invalid="ignore"):
        dev = np.where(want == 0.0, np.abs(got), np.abs(got - want) / np.abs(want))
    return float(dev.max()) if dev.size else 0.0


def check(scores, labels, status=None, cutoffs=CUT, alpha=20.0, bootstrap=0, seed=0):
    """One call against the restatement; returns (Enrichment, restatement)."""
    import torch

    from pharmaconet_amd import validation

    en = run(scores, labels, status, cutoffs, alpha, bootstrap, seed)
    host = scores.cpu().numpy() if isinstance(scores, torch.Tensor) else np.asarray(scores, dtype=np.float32)
    want = ref.enrichment_ref(host, labels, status, validation.cutoffs_ppm(cutoffs), alpha, bootstrap, seed)
    assert (en.totals == want["totals"]).all()
    assert (en.u2 == want["u2"]).all()
    assert en.order.shape == want["order"].shape and (en.order == want["order"]).all()
    assert (bits(en.hits) == bits(want["hits"])).all()
    dev = expsum_deviation(en.expsum, want["expsum"])
    print(f"expsum: largest relative deviation {dev:.3e} (n = {host.shape[-1]}, rows = {1 + bootstrap})")
    assert dev <= EXPSUM_RTOL
    return en, want


def tied_list(rng, n, actives=0.1, uncounted=0.0):
    """Scores with ties (about three ligands per value) and labels."""
    scores = rng.integers(0, n // 3 + 1, n).astype(np.float32) * np.float32(0.125)
    labels = rng.choice(np.array([0, 1, 2], dtype=np.uint8), n, p=(1.0 - actives - uncounted, actives, uncounted))
    return scores, labels


def sizes():
    t = 2048  # (collection happens without the package built: test_tile_constant holds this to the exported constant)
    return [1, 2, 255, 256, 257, 1023, 1024, 1025, t - 1, t, t + 1, 4095, 4096, 4097, 3 * t + 5]


def test_tile_constant():
    assert tile() == 2048 and set(sizes()) >= {tile() - 1, tile(), tile() + 1, 3 * tile() + 5}


@pytest.mark.parametrize("n", sizes())
def test_sizes_around_the_tile(n):
    rng = np.random.default_rng(n)
    scores, labels = tied_list(rng, n, actives=0.2, uncounted=0.05)
    check(scores, labels, bootstrap=1, seed=n)
    if n > 2:  # no ties at all: a group ends at every position, the tile's last one included
        check(rng.permutation(n).astype(np.float32), labels, bootstrap=1, seed=n + 1)


def test_one_group_over_several_tiles():
    rng = np.random.default_rng(1)
    t = tile()
    assert 5000 >= 2 * t + 2  # the group covers a whole tile and parts of both neighbours wherever it starts
    scores = np.concatenate([rng.random(700).astype(np.float32) + 1.0, np.zeros(5000, np.float32), -rng.random(300).astype(np.float32) - 1.0])
    labels = (rng.random(6000) < 0.1).astype(np.uint8)
    assert labels[700:5700].sum() > 100  # actives inside the group
    perm = rng.permutation(6000)
    en, _ = check(scores[perm], labels[perm], bootstrap=2, seed=3)
    assert 0.0 < en.auroc[0] < 1.0


@pytest.mark.parametrize("first", ["one group", "singletons"])
def test_group_boundary_on_a_tile_boundary(first):
    rng = np.random.default_rng(2)
    t = tile()
    head = np.full(t, 1000.0, np.float32) if first == "one group" else 5000.0 - np.arange(t, dtype=np.float32)
    scores = np.concatenate([head, np.full(7, 900.0, np.float32), 800.0 - np.arange(t + 3, dtype=np.float32)])  # positions t .. start a group
    labels = (rng.random(len(scores)) < 0.3).astype(np.uint8)
    en, want = check(scores, labels, bootstrap=1, seed=4)  # (already in rank order: position = ligand index)
    assert (want["order"][0] == np.arange(len(scores))).all()


def test_cutoffs_on_and_inside_groups():
    scores = np.concatenate([np.full(10, 3.0, np.float32), np.full(90, 2.0, np.float32), np.full(900, 1.0, np.float32)])
    labels = np.zeros(1000, np.uint8)
    labels[[0, 3, 7, 20, 50, 99, 400, 401, 999]] = 1
    en, _ = check(scores, labels, cutoffs=(0.01, 0.05, 1.0))  # k = 10: the first group's end; k = 50: inside the second; k = 1000: the list's end
    assert en.hits[0, 0].tolist() == [3.0, 3.0 + 3.0 * 40.0 / 90.0, 9.0]
    check(scores, labels, cutoffs=(0.01, 0.05, 1.0), bootstrap=3, seed=9)
    # 64 cutoffs, unsorted
    rng = np.random.default_rng(5)
    check(scores, labels, cutoffs=tuple(rng.integers(1, 1000001, 64) / 1e6), bootstrap=1, seed=2)


def test_special_values_and_status():
    rng = np.random.default_rng(6)
    n = 600
    scores = rng.integers(-3, 4, n).astype(np.float32)
    scores[rng.random(n) < 0.15] = -0.0
    scores[rng.random(n) < 0.1] = np.nan
    scores[rng.random(n) < 0.05] = np.inf
    scores[rng.random(n) < 0.05] = -np.inf
    status = np.where(rng.random(n) < 0.1, rng.integers(1, 5, n), 0).astype(np.int32)
    labels = (rng.random(n) < 0.3).astype(np.uint8)
    en, want = check(scores, labels, status, bootstrap=2, seed=8)
    key = ref.canonical(scores, status)
    zeros = np.flatnonzero(key == 0.0)
    assert np.signbit(scores[zeros]).any() and not np.signbit(scores[zeros]).all()  # -0.0 beside +0.0 ...
    pos = np.flatnonzero(np.isin(en.order[0], zeros))
    assert (np.diff(pos) == 1).all() and (np.diff(en.order[0][pos]) > 0).all()  # ... are one group, in index order
    last = en.order[0][-int((key == -np.inf).sum()):]
    assert (key[last] == -np.inf).all() and (np.diff(last) > 0).all()  # NaN, -inf and a non-zero status: last, tied
    check(scores, labels, None, bootstrap=1, seed=8)


def test_uncounted_and_degenerate_lists():
    rng = np.random.default_rng(7)
    scores, labels = tied_list(rng, 3000, actives=0.1, uncounted=0.4)
    en, want = check(scores, labels, bootstrap=2, seed=1)
    assert en.order.shape[1] == int((labels < 2).sum()) < 3000
    kept = labels < 2  # label 2 is the same as not being in the list - for the sample; a resample draws by ligand index
    sub = run(scores[kept], labels[kept])
    assert (sub.u2[:, 0] == en.u2[:, 0]).all() and (bits(sub.hits[:, 0]) == bits(en.hits[:, 0])).all() and (sub.totals[0] == en.totals[0]).all()
    for lab in (np.full(50, 2, np.uint8), np.zeros(50, np.uint8), np.ones(50, np.uint8)):  # nothing counted, no active, no decoy
        en, _ = check(scores[:50], lab, bootstrap=1, seed=2)
        assert np.isnan(en.auroc).all() and np.isnan(en.ef).all() and np.isnan(en.bedroc).all()
        assert en.ci("auroc") == pytest.approx((np.nan, np.nan, 0), nan_ok=True)


def test_refusals():
    import torch

    from pharmaconet_amd import _ffi, engine

    scores = torch.zeros(10, dtype=torch.float32, device="cuda")
    labels = np.zeros(10, np.uint8)
    with pytest.raises(ValueError, match="float64 scores are ranked by the caller"):
        engine.enrichment(scores.double(), labels)
    with pytest.raises(ValueError):
        engine.enrichment(scores, np.full(10, 3, np.uint8))
    with pytest.raises(_ffi.PmxError, match="labels other than"):
        engine.enrichment(scores, torch.full((10,), 3, dtype=torch.uint8, device="cuda"))  # a device tensor: refused by the call itself
    with pytest.raises(ValueError):
        engine.enrichment(scores, labels[:9])
    with pytest.raises(ValueError):
        engine.enrichment(scores, labels, cutoffs=(0.0,))
    with pytest.raises(ValueError):
        engine.enrichment(scores, labels, bootstrap=4097)
    lib = _ffi.load()
    assert lib.pmx_enrichment(None, 0, 1, 1, None, None, None, 0, 20.0, 0, 0, None, None, None, None, None, 0, 0, None) == 1
    assert b"pmx_enrichment" in lib.pmx_last_error()


@pytest.fixture(scope="module")
def three_columns():
    """n = 3 T + 5, three columns inside a wider buffer (col_stride > n), one list of labels."""
    import torch

    rng = np.random.default_rng(8)
    n = 3 * tile() + 5
    wide = torch.zeros((3, n + 11), dtype=torch.float32, device="cuda")
    host = np.stack([tied_list(rng, n)[0], rng.permutation(n).astype(np.float32), np.round(rng.normal(size=n), 2).astype(np.float32)])
    wide[:, :n] = torch.from_numpy(host).cuda()
    labels = rng.choice(np.array([0, 1, 2], dtype=np.uint8), n, p=(0.85, 0.1, 0.05))
    return wide[:, :n], host, labels


@pytest.mark.parametrize("bootstrap, seed", [(0, 0), (1, 1), (33, 1), (33, 2**63 + 12345)])
def test_columns_rows_and_seeds(three_columns, bootstrap, seed):
    view, host, labels = three_columns
    assert view.stride(0) > view.shape[1]
    en, _ = check(view, labels, bootstrap=bootstrap, seed=seed)
    assert en.u2.shape == (3, 1 + bootstrap) and en.hits.shape == (3, 1 + bootstrap, len(CUT))
    again = run(view, labels, bootstrap=bootstrap, seed=seed)  # two calls: identical bits
    for a, b in ((en.totals, again.totals), (en.u2, again.u2), (bits(en.hits), bits(again.hits)), (bits(en.expsum), bits(again.expsum)), (en.order, again.order)):
        assert (a == b).all()
    if bootstrap == 33:
        # a ligand's count is the same in every column: each column alone, under the seed, gives that column's rows (and the same totals)
        for c in range(3):
            one = run(host[c], labels, bootstrap=bootstrap, seed=seed, order=False)
            assert (one.totals == en.totals).all() and (one.u2[0] == en.u2[c]).all() and (bits(one.hits[0]) == bits(en.hits[c])).all()
            assert (bits(one.expsum[0]) == bits(en.expsum[c])).all()
        other = run(view, labels, bootstrap=bootstrap, seed=seed + 1, order=False)
        assert (other.totals[0] == en.totals[0]).all() and (other.totals[1:] != en.totals[1:]).any()  # the seed moves the resamples only
        d = en.delta(0, 2, "auroc")
        assert d["n"] == 33 and d["low"] <= d["high"] and 0.0 <= d["share"] <= 1.0
        low, high, used = en.ci("bedroc", 1)
        assert used == 33 and low <= high


def test_order_inside_tie_groups_has_no_effect():
    rng = np.random.default_rng(9)
    n = 2 * tile() + 77
    scores, labels = tied_list(rng, n, actives=0.15, uncounted=0.05)
    scores[rng.random(n) < 0.3] = 0.0  # one large group among the small ones
    perm = np.arange(n)
    for v in np.unique(scores):  # shuffle the ligand indices inside every group: which of them come first changes, the groups do not
        where = np.flatnonzero(scores == v)
        perm[where] = rng.permutation(where)
    assert (scores[perm] == scores).all() and (labels[perm] != labels).any()
    a, b = run(scores, labels), run(scores[perm], labels[perm])
    assert (a.totals == b.totals).all() and (a.u2 == b.u2).all() and (bits(a.hits) == bits(b.hits)).all() and (bits(a.expsum) == bits(b.expsum)).all()
    assert (scores[perm][b.order[0]] == scores[a.order[0]]).all()  # (both orders rank the same values)


def test_call_on_a_side_stream_follows_the_producer():
    import torch

    rng = np.random.default_rng(10)
    n = 3 * tile() + 5
    base = torch.from_numpy(rng.normal(size=n).astype(np.float32)).cuda()
    labels = (rng.random(n) < 0.1).astype(np.uint8)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        x = base
        for _ in range(200):  # the producer: work that is still running when the call is enqueued behind it
            x = torch.sin(x) * 1.25 + 0.125
        scores = torch.round(x * 8.0) / 8.0
        on_side, _ = check(scores, labels, bootstrap=2, seed=5)
    # the next call, on the default stream, shares the work buffers: it starts behind the one before
    side.synchronize()
    on_default, _ = check(scores, labels, bootstrap=2, seed=5)
    assert (on_side.u2 == on_default.u2).all() and (bits(on_side.expsum) == bits(on_default.expsum)).all()


# ---------------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def golden_screen():
    model, lib, weights, _ = load_golden("set_6oim_c8")
    from pharmaconet_amd.engine import DeviceLibrary

    dlib = DeviceLibrary(lib)
    labels = (np.random.default_rng(11).random(len(lib)) < 0.2).astype(np.uint8)
    return model, dlib, weights, labels, model.screen(dlib, weights=weights)


def test_screening_result_enrichment(golden_screen):
    from pharmaconet_amd import validation

    model, dlib, weights, labels, result = golden_screen
    en = result.enrichment(labels, bootstrap=5, seed=3, order=True)
    want = ref.enrichment_ref(result.scores.cpu().numpy(), labels, result.status.cpu().numpy(), validation.cutoffs_ppm((0.005, 0.01, 0.05)), 20.0, 5, 3)
    assert (en.totals == want["totals"]).all() and (en.u2 == want["u2"]).all() and (en.order == want["order"]).all()
    assert (bits(en.hits) == bits(want["hits"])).all() and expsum_deviation(en.expsum, want["expsum"]) <= EXPSUM_RTOL
    n, na, nd = (int(v) for v in want["totals"][0])
    assert en.n_active == na == int(labels.sum()) and en.n_decoy == nd
    assert en.auroc[0] == ref.auroc(want["u2"][0, 0], na, nd)
    assert en.bedroc[0] == pytest.approx(ref.bedroc(want["expsum"][0, 0], n, na, nd, 20.0), rel=1e-10)
    with pytest.raises(ValueError, match="float64 scores are ranked by the caller"):
        model.screen(dlib, weights=weights, float64=True).enrichment(labels)
    from pharmaconet_amd.engine import screen_multi

    panel = screen_multi([model, model], dlib, weights=weights).enrichment(labels, bootstrap=5, seed=3)
    assert (panel.u2[0] == en.u2[0]).all() and (panel.u2[1] == en.u2[0]).all() and panel.delta(0, 1, "auroc")["value"] == 0.0


def test_sweep_columns_are_screens(golden_screen):
    from pharmaconet_amd import engine

    model, dlib, weights, labels, result = golden_screen
    other = dict(Cation=8.0, Anion=8.0, Aromatic=1.0, HBond_donor=4.0, HBond_acceptor=2.0, Halogen=4.0, Hydrophobic=3.0)
    sets = [None, other]
    en, scores = engine.sweep([model], dlib, labels, sets, bootstrap=7, seed=4, return_scores=True)
    assert en.columns == [(0, 0), (0, 1)] and tuple(scores.shape) == (2, len(labels))
    differ = False
    for w, ws in enumerate(sets):
        single = model.screen(dlib, weights=ws)
        assert (scores[w].cpu().numpy().view(np.uint32) == single.scores.cpu().numpy().view(np.uint32)).all()  # no score moves
        one = single.enrichment(labels, bootstrap=7, seed=4)
        assert (one.totals == en.totals).all()  # the resample counts are per ligand, not per column
        assert (one.u2[0] == en.u2[w]).all() and (bits(one.hits[0]) == bits(en.hits[w])).all() and (bits(one.expsum[0]) == bits(en.expsum[w])).all()
        assert one.auroc[0] == en.auroc[w] and (one.ef[0] == en.ef[w]).all() and one.bedroc[0] == en.bedroc[w]
        differ |= w > 0 and bool((scores[w] != scores[0]).any())
    assert differ
    assert model.sweep(dlib, labels, sets).auroc.tolist() == en.auroc.tolist()
    d = en.delta((0, 1), (0, 0), "auroc")
    assert d["n"] <= 7 and d["value"] == en.auroc[1] - en.auroc[0]


def test_cli_enrichment_out(tmp_path, golden_screen):
    from pharmaconet_amd.screening import main

    model, dlib, weights, labels, result = golden_screen
    _, lib, _, _ = load_golden("set_6oim_c8")
    libfile = tmp_path / "lib.pmxlib"
    lib.save(libfile)
    (tmp_path / "lib.pmxlib.names").write_text("\n".join(f"/data/mol_{i}.sdf" for i in range(len(lib))))
    actives = tmp_path / "actives.txt"
    actives.write_text("".join(f"mol_{i}\n" if i % 2 else f"/data/mol_{i}.sdf\n" for i in np.flatnonzero(labels)))
    base = ["-p", str(GOLDEN / "model_6oim_like.pm"), "-d", str(libfile)]
    main(base + ["-o", str(tmp_path / "plain.csv")])
    main(base + ["-o", str(tmp_path / "out.csv"), "--actives", str(actives), "--enrichment_out", str(tmp_path / "e.csv"), "--bootstrap", "20", "--bootstrap_seed", "6"])
    assert (tmp_path / "out.csv").read_bytes() == (tmp_path / "plain.csv").read_bytes()
    rows = [ln.split(",") for ln in (tmp_path / "e.csv").read_text().splitlines()]
    assert rows[0] == ["metric", "value", "ci_low", "ci_high"]
    assert [r[0] for r in rows[1:]] == ["n_active", "n_decoy", "auroc", "bedroc", "ef@0.005", "ef@0.01", "ef@0.05"]
    want = model.screen(dlib).enrichment(labels, bootstrap=20, seed=6)  # (the command line's default weights are the defaults)
    assert int(rows[1][1]) == int(labels.sum()) and float(rows[3][1]) == want.auroc[0] and float(rows[5][1]) == want.ef[0, 0]
    low, high, _ = want.ci("auroc")
    assert (float(rows[3][2]), float(rows[3][3])) == (low, high)
    main(base + ["-o", str(tmp_path / "out2.csv"), "--actives", str(actives), "--enrichment_out", str(tmp_path / "e0.csv")])
    assert all(r.split(",")[2:] == ["", ""] for r in (tmp_path / "e0.csv").read_text().splitlines()[1:])
    actives.write_text("mol_1\nmol_999999\n")
    with pytest.raises(SystemExit):
        main(base + ["-o", str(tmp_path / "err.csv"), "--actives", str(actives), "--enrichment_out", str(tmp_path / "x.csv")])
    with pytest.raises(SystemExit):
        main(base + ["-o", str(tmp_path / "err.csv"), "--actives", str(actives)])
