"""Retrospective validation without a GPU: the NumPy restatement of pmx_enrichment's specification (tests/enrichment_ref.py) held to a
brute force of the definitions and to closed cases, the Poisson table held to `decimal`, and the host layer (`Enrichment.ci`, `delta`,
the actives file of the command line) on hand-made inputs."""

import math
from decimal import Decimal, getcontext

import numpy as np
import pytest

import enrichment_ref as ref
from pharmaconet_amd import engine, validation
from pharmaconet_amd.validation import Enrichment, match_actives


# ------------------------------------------------------------------------------------------------------------ the generator
def test_poisson_table_against_decimal():
    getcontext().prec = 70
    e_inv = Decimal(1) / Decimal(1).exp()
    cdf, term, table = Decimal(0), Decimal(1), []
    for m in range(40):
        if m:
            term /= m
        cdf += term
        table.append(int(cdf * e_inv * (1 << 64)))  # (int() truncates: the value is positive)
        if table[-1] == (1 << 64) - 1:
            break
    assert len(table) == 21 and table[-1] == (1 << 64) - 1 and table[-2] < table[-1]
    assert list(engine.POISSON1_CDF64) == table
    assert ref.TABLE == table
    assert engine.POISSON1_CDF64 is validation.POISSON1_CDF64


def test_hash_vector_form_equals_integer_form_and_is_poisson():
    for seed, b in ((0, 1), (12345, 7), ((1 << 64) - 1, 4096)):
        c = ref.counts(seed, b, 300)
        assert [ref.count_int(seed, b, i) for i in range(300)] == c.tolist()
    assert (ref.counts(3, 0, 10) == 1).all()
    c = ref.counts(2024, 3, 200000)
    assert abs(c.mean() - 1.0) < 0.01 and abs(c.var() - 1.0) < 0.02
    assert abs((c == 0).mean() - math.exp(-1)) < 0.005
    assert (ref.counts(2024, 3, 1000) != ref.counts(2024, 4, 1000)).any()


# ------------------------------------------------------------------------------------------------------------ brute force
def brute(scores, labels, w, cut_ppm, alpha):
    """The definitions, O(n^2): every ligand i stands for w[i] copies of itself."""
    key = ref.canonical(scores)
    cnt = np.flatnonzero((labels < 2) & (w > 0))
    act, dec = [i for i in cnt if labels[i] == 1], [i for i in cnt if labels[i] == 0]
    u2 = 0
    for i in act:
        for j in dec:
            u2 += int(w[i]) * int(w[j]) * (2 if key[i] > key[j] else 1 if key[i] == key[j] else 0)
    items = sorted(((-key[i], int(labels[i])) for i in cnt for _ in range(int(w[i]))))  # one entry per copy, best first
    n_star = len(items)
    hits = []
    for ppm in cut_ppm:
        if n_star == 0:
            hits.append(0.0)
            continue
        k = -(-int(ppm) * n_star // 1000000)
        v = items[k - 1][0]  # the value the cutoff falls on
        above = [l for kv, l in items if kv < v]
        tied = [l for kv, l in items if kv == v]
        hits.append(sum(above) + sum(tied) * (k - len(above)) / len(tied))  # hypergeometric mean of the straddling group
    expsum, r = 0.0, 0
    while r < n_star:
        e = r
        while e < n_star and items[e][0] == items[r][0]:
            e += 1
        mean = sum(math.exp(-alpha * rank / n_star) for rank in range(r + 1, e + 1)) / (e - r)
        expsum += sum(l for _, l in items[r:e]) * mean
        r = e
    return u2, hits, expsum


def test_restatement_against_brute_force():
    rng = np.random.default_rng(20240611)
    cut_ppm = (5000, 10000, 50000, 333333, 1000000)
    for case in range(200):
        n = int(rng.integers(1, 201))
        levels = int(rng.integers(1, 8))
        scores = rng.integers(0, levels, n).astype(np.float32) * np.float32(0.25)  # heavy ties
        if case % 3 == 0:
            scores[rng.random(n) < 0.1] = np.nan
            scores[rng.random(n) < 0.1] = -0.0
        labels = rng.choice(np.array([0, 1, 2], dtype=np.uint8), n, p=(0.6, 0.3, 0.1))
        alpha = float(rng.choice([5.0, 20.0, 80.5]))
        seed, n_boot = int(rng.integers(0, 1 << 62)), 2
        out = ref.enrichment_ref(scores, labels, None, cut_ppm, alpha, n_boot, seed)
        for b in range(1 + n_boot):
            w = np.array([ref.count_int(seed, b, i) for i in range(n)])
            u2, hits, expsum = brute(scores, labels, w, cut_ppm, alpha)
            wc = np.where(labels < 2, w, 0)
            assert out["totals"][b].tolist() == [int(wc.sum()), int(wc[labels == 1].sum()), int(wc[labels == 0].sum())]
            assert int(out["u2"][0, b]) == u2
            np.testing.assert_allclose(out["hits"][0, b], hits, rtol=1e-13, atol=0)
            np.testing.assert_allclose(out["expsum"][0, b], expsum, rtol=1e-11, atol=0)


# ------------------------------------------------------------------------------------------------------------ closed cases
def metrics(out, cut_ppm, alpha, b=0, c=0):
    n, na, nd = (int(v) for v in out["totals"][b])
    return (ref.auroc(out["u2"][c, b], na, nd), [ref.ef(out["hits"][c, b, j], p, n, na, nd) for j, p in enumerate(cut_ppm)],
            ref.bedroc(out["expsum"][c, b], n, na, nd, alpha))


@pytest.mark.parametrize("n, n_a", [(1000, 10), (400, 100), (200, 1)])
def test_perfect_and_inverted_ranking(n, n_a):
    cut_ppm, alpha = (5000, 10000, 50000, 500000), 20.0
    labels = np.zeros(n, dtype=np.uint8)
    labels[:n_a] = 1
    scores = np.arange(n, 0, -1).astype(np.float32)
    auroc, ef, bedroc = metrics(ref.enrichment_ref(scores, labels, None, cut_ppm, alpha), cut_ppm, alpha)
    assert auroc == 1.0 and abs(bedroc - 1.0) < 1e-12
    for j, ppm in enumerate(cut_ppm):
        assert ppm * n % 1000000 == 0  # (f N is an integer: the closed form holds)
        assert abs(ef[j] - min(n / n_a, 1e6 / ppm)) < 1e-12 * (n / n_a)
    auroc, ef, bedroc = metrics(ref.enrichment_ref(-scores, labels, None, cut_ppm, alpha), cut_ppm, alpha)
    assert auroc == 0.0 and abs(bedroc) < 1e-12


def test_all_scores_equal():
    """AUROC exactly 0.5 and EF exactly 1 for the sample; in a resample the weighted counts are arbitrary integers and a k / N* need not be
    a double, so EF is 1 to the four roundings of its formula there (AUROC stays exact: it is a quotient of integers)."""
    cut_ppm, alpha = (5000, 10000, 50000, 1000000), 20.0
    for n, every in ((1000, 10), (997, 7), (200, 3)):
        lab = (np.arange(n) % every == 0).astype(np.uint8)
        out = ref.enrichment_ref(np.full(n, 0.5, np.float32), lab, None, cut_ppm, alpha, n_boot=3, seed=5)
        auroc, ef, bedroc = metrics(out, cut_ppm, alpha, 0)
        assert auroc == 0.5 and ef == [1.0] * 4
        for b in range(1, 4):
            auroc, ef, bedroc = metrics(out, cut_ppm, alpha, b)
            assert auroc == 0.5 and max(abs(e - 1.0) for e in ef) <= 4 * 2.0**-53
    labels = (np.arange(1000) % 10 == 0).astype(np.uint8)
    out = ref.enrichment_ref(np.full(1000, 0.5, np.float32), labels, None, cut_ppm, alpha)
    # one group: the order inside it has no effect, so neither has listing the actives first
    first = ref.enrichment_ref(np.full(1000, 0.5, np.float32), np.sort(labels)[::-1], None, cut_ppm, alpha)
    assert first["u2"][0, 0] == out["u2"][0, 0] and (first["hits"][0, 0] == out["hits"][0, 0]).all()


def test_degenerate_rows_are_nan():
    for labels in (np.zeros(5, np.uint8), np.ones(5, np.uint8), np.full(5, 2, np.uint8)):
        out = ref.enrichment_ref(np.arange(5, dtype=np.float32), labels, None, (500000,), 20.0)
        auroc, ef, bedroc = metrics(out, (500000,), 20.0)
        assert math.isnan(auroc) and math.isnan(ef[0]) and math.isnan(bedroc)
        en = Enrichment(totals=out["totals"], u2=out["u2"], hits=out["hits"], expsum=out["expsum"], cut_ppm=np.array([500000], np.uint32), alpha=20.0)
        assert np.isnan(en.auroc).all() and np.isnan(en.ef).all() and np.isnan(en.bedroc).all()


# ------------------------------------------------------------------------------------------------------------ the host layer
def test_enrichment_formulas_equal_the_restatement():
    rng = np.random.default_rng(7)
    scores = np.round(rng.normal(size=(2, 500)), 1).astype(np.float32)
    labels = (rng.random(500) < 0.1).astype(np.uint8)
    cut = (0.005, 0.01, 0.05)
    ppm = validation.cutoffs_ppm(cut)
    assert ppm.tolist() == [5000, 10000, 50000]
    out = ref.enrichment_ref(scores, labels, None, ppm, 20.0, n_boot=4, seed=11)
    en = Enrichment(totals=out["totals"], u2=out["u2"], hits=out["hits"], expsum=out["expsum"], cut_ppm=ppm, alpha=20.0)
    assert en.n_active == int(labels.sum()) and en.n_decoy == 500 - int(labels.sum()) and en.n_resamples == 4
    for c in range(2):
        for b in range(5):
            auroc, ef, bedroc = metrics(out, ppm, 20.0, b, c)
            assert en.auroc_rows()[c, b] == auroc
            np.testing.assert_allclose(en.ef_rows()[c, b], ef, rtol=1e-15)
            np.testing.assert_allclose(en.bedroc_rows()[c, b], bedroc, rtol=1e-13)
    assert en.metric_names() == ["auroc", "bedroc", "ef@0.005", "ef@0.01", "ef@0.05"]
    assert (en.metric_rows("ef@0.01") == en.ef_rows()[:, :, 1]).all()
    with pytest.raises(ValueError):
        en.metric_rows("ef@0.02")
    with pytest.raises(ValueError):
        validation.cutoffs_ppm([0.0])


def handmade(auroc_a, auroc_b):
    """Two columns whose AUROC rows are the given values (row 0 first): 5 actives and 5 decoys in every row, u2 = 50 AUROC."""
    rows = len(auroc_a)
    totals = np.tile(np.array([10, 5, 5], dtype=np.uint64), (rows, 1))
    u2 = np.array([[round(50 * v) for v in auroc_a], [round(50 * v) for v in auroc_b]], dtype=np.uint64)
    return Enrichment(totals=totals, u2=u2, hits=np.zeros((2, rows, 0)), expsum=np.zeros((2, rows)), cut_ppm=np.zeros(0, np.uint32), alpha=20.0, columns=[(0, 0), (0, 1)])


def test_ci_and_delta_on_handmade_resamples():
    a = [0.8] + [0.5 + 0.02 * i for i in range(21)]  # resamples 0.50, 0.52 ... 0.90
    b = [0.6] + [0.7] * 21
    en = handmade(a, b)
    low, high, n = en.ci("auroc", 0, level=0.9)
    assert n == 21 and abs(low - 0.52) < 1e-12 and abs(high - 0.88) < 1e-12  # 5th and 95th percentile of 21 evenly spaced values
    assert en.ci("auroc", (0, 1)) == (0.7, 0.7, 21)
    d = en.delta((0, 0), (0, 1), "auroc", level=0.9)
    assert abs(d["value"] - 0.2) < 1e-12 and d["n"] == 21
    assert abs(d["low"] + 0.18) < 1e-12 and abs(d["high"] - 0.18) < 1e-12
    assert abs(d["share"] - 10 / 21) < 1e-12  # 0.72 ... 0.90 beat 0.70; the tie at 0.70 does not
    # a resample without actives is NaN: left out, and counted out
    en.totals[3] = (10, 0, 10)
    assert math.isnan(en.auroc_rows()[0, 3]) and en.ci("auroc", 0)[2] == 20 and en.delta(0, 1, "auroc")["n"] == 20
    none = handmade([0.8], [0.6])
    assert none.ci("auroc")[2] == 0 and math.isnan(none.ci("auroc")[0]) and math.isnan(none.delta(0, 1, "auroc")["share"])
    with pytest.raises(ValueError):
        en.ci("auroc", 0, level=1.5)


def test_actives_file_matching():
    names = ["/lib/a/lig1.sdf", "/lib/a/lig2.sdf", "/lib/b/lig3.mol2", "plain", "/lib/c/lig2.sdf"]
    assert match_actives(["lig1", "", "  /lib/b/lig3.mol2  ", "plain"], names).tolist() == [1, 0, 1, 1, 0]
    assert match_actives(["/lib/c/lig2.sdf"], names).tolist() == [0, 0, 0, 0, 1]  # exact wins over the ambiguous stem
    assert match_actives(["lig3.mol2"], names).tolist() == [0, 0, 1, 0, 0]
    with pytest.raises(ValueError, match=r"2 line\(s\).*nope, neither"):
        match_actives(["lig1", "nope", "neither"], names)
    with pytest.raises(ValueError, match="twice.*lig2"):
        match_actives(["lig2"], names)  # the stem names two ligands
    with pytest.raises(ValueError, match="twice.*lig1"):
        match_actives(["lig1", "/lib/a/lig1.sdf"], names)
    many = [f"x{i}" for i in range(9)]
    with pytest.raises(ValueError, match=r"x0, x1, x2, x3, x4 \.\.\."):
        match_actives(many, names)


def test_enrichment_csv(tmp_path):
    en = handmade([0.8] + [0.5 + 0.02 * i for i in range(21)], [0.6] + [0.7] * 21)
    validation.write_enrichment_csv(tmp_path / "e.csv", en)
    lines = (tmp_path / "e.csv").read_text().splitlines()
    assert lines[:3] == ["metric,value,ci_low,ci_high", "n_active,5,,", "n_decoy,5,,"]
    name, value, low, high = lines[3].split(",")
    assert name == "auroc" and float(value) == 0.8 and float(low) < 0.8 < float(high)
    validation.write_enrichment_csv(tmp_path / "e0.csv", handmade([0.8], [0.6]))
    assert (tmp_path / "e0.csv").read_text().splitlines()[3] == "auroc,0.8,,"


def test_command_line_knows_the_flags():
    from pharmaconet_amd.screening import Screening_ArgParser

    args = Screening_ArgParser().parse_args(["-p", "m.pm", "-d", "lib", "-o", "out.csv", "--actives", "a.txt", "--enrichment_out", "e.csv", "--bootstrap", "100"])
    assert args.enrichment_cut == "0.5,1,5" and args.bedroc_alpha == 20.0 and args.bootstrap == 100 and args.bootstrap_seed == 0
    assert callable(engine.enrichment) and callable(engine.sweep)
