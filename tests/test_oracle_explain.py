"""`oracle_explain` (oracle/pmx_oracle.c) against the reference's own leaves: the per-conformer maxima and keys of tests/golden/explain_<set>.npz,
the filtered ones of constrained_<set>.npz and the ranked lists of modes_<set>.npz, under the rules the GPU fixture tests use (values within
2e-6, levels and n_positive exact, a key exact wherever the fixture's gap is above 1e-5, else a key whose `path_score` is the value). This is
what pins the entry point; tests/test_gpu_explain_shapes.py then uses it as the reference at the shapes no fixture covers."""

import functools

import numpy as np
import pytest

from conftest import GOLDEN_SETS, load_golden
from constrained_ref import CONSTRAINED_SETS
from explain_ref import NONE, Tables, path_score
from modes_ref import MODES_SETS

RTOL = 2e-6  # test_gpu_parity.py's RTOL, the bar of the explain, constrained and modes fixture tests
TIE = 1e-5
EXPLAIN_SETS = ("set_6oim_c8", "set_6oim_c1", "set_6oim_c64", "set_c21_c8", "set_6oim_c8_weights", "set_s64_c8")
THREADS = 8


@functools.lru_cache(maxsize=None)
def walked(name):
    """(model, library, weights7, oracle_explain of the whole set at n_modes = 8, oracle_score of the whole set)."""
    from oracle import oracle
    from pharmaconet_amd.constants import weights_vector

    model, lib, weights, _ = load_golden(name)
    w7 = weights_vector(weights)
    out = oracle.oracle_explain(model.flat, lib, w7, n_modes=8, num_threads=THREADS)
    return model, lib, w7, out, oracle.oracle_score(model.flat, lib, w7, num_threads=THREADS)


def as_key(raw, nl):
    key = raw[..., :nl].astype(np.int64)
    key[key == 0xFF] = NONE
    return key


def check_levels(out_levels, lv):
    nl = len(lv)
    assert out_levels[:nl].tolist() == lv.tolist() and (out_levels[nl:] == 0xFE).all()


def key_reaches(model, lib, w7, i, lv, key, c, value, cache):
    """A key within the tie band is accepted by its total: `path_score` of it is the value within 2e-6."""
    if i not in cache:
        rec = lib.unpack(i)
        cache[i] = (rec, Tables(model, rec, w7))
    rec, T = cache[i]
    return abs(path_score(model, rec, w7, lv, key, c, T) - value) <= RTOL * value


@pytest.mark.parametrize("name", GOLDEN_SETS)
def test_mode_0_means_are_oracle_score_bit_for_bit(name, oracle):
    """Every ligand of every golden set: the mean of mode 0 (summed in conformer order, as `score_ligand` does) is `oracle_score`'s float64,
    the walk's own `scores` output likewise, the lists are sorted, and entries past a list's end are 0 / 0xFF."""
    _, lib, _, out, scores = walked(name)
    assert np.array_equal(out["scores"], scores)
    for i in range(len(lib)):
        C = lib.header(i)[1]
        total = 0.0
        for v in out["values"][i, 0, :C]:
            total += float(v)
        assert total / C == scores[i], (name, i)
        assert (out["values"][i, :, C:] == 0).all() and (out["keys"][i, :, C:] == 0xFF).all() and (out["n_positive"][i, C:] == 0).all()
    v = out["values"]
    assert (np.diff(v, axis=1) <= 0).all()
    held = np.arange(8)[None, :, None] < out["n_positive"][:, None, :]
    assert np.array_equal(v > 0, held)
    assert (out["keys"][~held] == 0xFF).all()


def test_one_mode_is_the_head_of_eight(oracle):
    """n_modes = 1 keeps what n_modes = 8 keeps first, bit for bit, and counts the same leaves."""
    from oracle import oracle as o

    model, lib, w7, out, _ = walked("set_c21_c8")
    one = o.oracle_explain(model.flat, lib, w7, n_modes=1, num_threads=THREADS)
    assert np.array_equal(one["values"][:, 0], out["values"][:, 0]) and np.array_equal(one["keys"][:, 0], out["keys"][:, 0])
    assert np.array_equal(one["n_positive"], out["n_positive"]) and np.array_equal(one["levels"], out["levels"])
    assert np.array_equal(one["scores"], out["scores"])


@pytest.mark.parametrize("name", EXPLAIN_SETS)
def test_reference_explain_fixtures(name, oracle):
    from test_explain_cpu import fixture_rows, load_explain

    model, lib, w7, out, _ = walked(name)
    x = load_explain(name)[4]
    exact, cache = 0, {}
    for i, C, lv, sc, key, gap in fixture_rows(x):
        check_levels(out["levels"][i], lv)
        got_v, got_k = out["values"][i, 0, :C], as_key(out["keys"][i, 0, :C], len(lv))
        assert np.allclose(got_v, sc, rtol=RTOL, atol=0), (name, i)
        assert np.array_equal(got_v == 0, sc == 0)
        assert (out["keys"][i, 0, :, len(lv):] == 0xFF).all()
        for c in range(C):
            if sc[c] <= 0:
                assert (got_k[c] == NONE).all() and out["n_positive"][i, c] == 0
            elif gap[c] > TIE:
                assert got_k[c].tolist() == key[c].tolist(), (name, i, c)
                exact += 1
            else:
                assert key_reaches(model, lib, w7, i, lv, got_k[c], c, sc[c], cache), (name, i, c)
    assert exact > 0


@pytest.mark.parametrize("name", CONSTRAINED_SETS)
def test_reference_constrained_fixtures(name, oracle):
    from constrained_ref import fixture_rows, load_constrained, qualifies
    from oracle import oracle as o

    model, lib, w7, _, _ = walked(name)
    x = load_constrained(name)[4]
    exact, cache = 0, {}
    for i, _, C, lv, require, exclude, sc, key, gap, unc in fixture_rows(x):
        out = o.oracle_explain(model.flat, lib, w7, first=i, count=1, n_modes=1, constraint=(require, exclude))
        check_levels(out["levels"][0], lv)
        got_v, got_k = out["values"][0, 0, :C], as_key(out["keys"][0, 0, :C], len(lv))
        assert np.allclose(got_v, sc, rtol=RTOL, atol=0), (name, i, require, exclude)
        assert np.array_equal(got_v == 0, sc == 0) and (got_v <= unc * (1 + RTOL)).all()
        for c in range(C):
            if sc[c] <= 0:
                assert (got_k[c] == NONE).all() and out["n_positive"][0, c] == 0
                continue
            assert qualifies(got_k[c], require, exclude)
            if gap[c] > TIE:
                assert got_k[c].tolist() == key[c].tolist(), (name, i, c, require, exclude)
                exact += 1
            else:
                assert key_reaches(model, lib, w7, i, lv, got_k[c], c, sc[c], cache), (name, i, c)
    assert exact > 0, name


@pytest.mark.parametrize("name", MODES_SETS)
def test_reference_modes_fixtures(name, oracle):
    from modes_ref import MAX_MODES, fixture_rows, key_exact, load_modes

    model, lib, w7, out, _ = walked(name)
    x = load_modes(name)[4]
    exact, cache = 0, {}
    for i, C, lv, values, key, gap, n_positive in fixture_rows(x):
        check_levels(out["levels"][i], lv)
        got_v, got_k = out["values"][i, :, :C], as_key(out["keys"][i, :, :C], len(lv))
        assert np.allclose(got_v, values, rtol=RTOL, atol=0), (name, i)
        assert np.minimum(out["n_positive"][i, :C], 255).tolist() == n_positive.tolist(), (name, i)  # (the fixture caps the count at 255)
        for m in range(MAX_MODES):
            for c in range(C):
                if m >= n_positive[c]:
                    assert got_v[m, c] == 0 and (got_k[m, c] == NONE).all()
                elif key_exact(gap, m, c):
                    assert got_k[m, c].tolist() == key[m, c].tolist(), (name, i, m, c)
                    exact += 1
                else:
                    assert key_reaches(model, lib, w7, i, lv, got_k[m, c], c, values[m, c], cache), (name, i, m, c)
    assert exact > 0, name


def test_a_constraint_per_ligand_and_the_refusals(oracle):
    """`constraints=` gives each ligand its own: row by row the answer of a one-constraint call. n_modes outside 1 .. 8 is refused."""
    from oracle import oracle as o

    model, lib, w7, out, _ = walked("set_c21_c8")
    rng = np.random.default_rng(7)
    K = model.flat.num_clusters
    cons = [([sorted({int(a) for a in rng.integers(0, K, 2)})], [int(rng.integers(0, K))] if r % 2 else []) for r in range(12)]
    many = o.oracle_explain(model.flat, lib, w7, first=3, count=12, n_modes=3, constraints=cons, num_threads=4)
    changed = 0
    for r, con in enumerate(cons):
        one = o.oracle_explain(model.flat, lib, w7, first=3 + r, count=1, n_modes=3, constraint=con)
        for k in one:
            assert np.array_equal(one[k][0], many[k][r]), (r, k)
        assert (many["values"][r, 0] <= out["values"][3 + r, 0]).all() and (many["n_positive"][r] <= out["n_positive"][3 + r]).all()
        changed += not np.array_equal(many["values"][r, 0], out["values"][3 + r, 0])
    assert changed > 0
    for bad in (0, 9):
        with pytest.raises(RuntimeError):
            o.oracle_explain(model.flat, lib, w7, count=1, n_modes=bad)
