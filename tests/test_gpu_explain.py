"""`pmx_explain` on the GPU (csrc/pmx_explain.hip): per-conformer maxima and the leaf that reaches each, checked against the
reference's recorded scores, the NumPy restatement of tests/explain_ref.py and the product's own score pass."""

import numpy as np
import pytest

from conftest import GOLDEN_SETS, load_golden
from explain_ref import Tables, first_max_key, path_score, tree_leaves

pytestmark = pytest.mark.gpu


def ulp_close(a, b, n=4):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) <= n * np.spacing(np.maximum(np.abs(a), np.abs(b)))


def check_against_score_pass(model, lib, weights, idx, n_path=64):
    """Means of the maxima = pmx_score_f64 (<= 4 ulp), no miss, and path_score of reported keys = their maxima (first n_path ligands)."""
    from pharmaconet_amd.constants import weights_vector
    from pharmaconet_amd.engine import explain, screen

    idx = np.asarray(idx, dtype=np.int64)
    res = screen(model, lib, weights=weights, float64=True)
    sc, st = res.scores.cpu().numpy(), res.status.cpu().numpy()
    ex = explain(model, lib, idx, weights=weights)
    assert not (ex.status == 3).any()
    assert np.array_equal(ex.status, st[idx])
    w7 = weights_vector(weights)
    for r, i in enumerate(idx):
        if ex.status[r] != 0:
            assert np.isnan(ex.conf_max[r]).all() and ex.best_conformer[r] == -1
            continue
        cm = ex.conf_max[r]
        assert ulp_close(cm.mean(), sc[i]), (i, cm.mean(), sc[i])
        assert ex.best_conformer[r] == int(np.argmax(cm))
        if r < n_path:
            rec = lib.unpack(int(i))
            T = Tables(model, rec, w7)
            for c in range(len(cm)):
                key = ex.match[r][c]
                if cm[c] > 0:
                    assert abs(path_score(model, rec, w7, ex.levels[r], key, c, T) - cm[c]) <= 2e-6 * cm[c], (i, c)
                else:
                    assert (key == -1).all()
    return ex


@pytest.mark.parametrize("name", ("set_6oim_c8", "set_6oim_c1", "set_6oim_c64", "set_c21_c8", "set_6oim_c8_weights", "set_s64_c8"))
def test_reference_explain_fixtures(name):
    """tests/golden/explain_<set>.npz (the reference's own tree search): maxima within 2e-6, levels and best conformer exact, the key
    exact wherever the runner-up with another key is more than 1e-5 below, else a key whose path_score is the maximum."""
    from pharmaconet_amd.constants import weights_vector
    from pharmaconet_amd.engine import explain
    from test_explain_cpu import fixture_rows, load_explain

    model, lib, weights, _, x = load_explain(name)
    w7 = weights_vector(weights)
    rows = list(fixture_rows(x))
    ex = explain(model, lib, [r[0] for r in rows], weights=weights)
    exact = 0
    for r, (i, C, lv, sc, key, gap) in enumerate(rows):
        assert ex.status[r] == 0
        assert np.allclose(ex.conf_max[r], sc, rtol=2e-6, atol=0), (i, ex.conf_max[r], sc)
        assert ex.levels[r].tolist() == lv.tolist()
        assert ex.best_conformer[r] == int(np.argmax(sc))
        rec, T = None, None
        for c in range(C):
            got = ex.match[r][c]
            if sc[c] <= 0:
                assert (got == -1).all()
            elif gap[c] > 1e-5:
                assert got.tolist() == key[c].tolist(), (i, c)
                exact += 1
            else:
                if T is None:
                    rec = lib.unpack(i)
                    T = Tables(model, rec, w7)
                assert abs(path_score(model, rec, w7, lv, got, c, T) - sc[c]) <= 2e-6 * sc[c], (i, c)
    assert exact > 0


@pytest.mark.parametrize("name", GOLDEN_SETS)
def test_golden_sets(name):
    """Every golden ligand: maxima average to the reference's score, levels as the reference counts them, keys reproduce the maxima."""
    from pharmaconet_amd.engine import explain

    model, lib, weights, d = load_golden(name)
    idx = np.arange(len(lib))
    ex = check_against_score_pass(model, lib, weights, idx, n_path=32 if "l110" not in name else 4)
    ref = d["score"]
    for r in range(len(lib)):
        if ex.status[r] == 0:
            assert abs(ex.conf_max[r].mean() - ref[r]) <= 2e-6 * max(abs(ref[r]), 1e-30) + 1e-12, r
            assert len(ex.levels[r]) == int(d["n_levels"][r])
    assert ex.max.shape == (len(lib),)


@pytest.mark.parametrize("name", ("set_6oim_c1", "set_6oim_c8", "set_6oim_c8_weights", "set_c21_c8", "set_6oim_c64", "set_s64_c8"))
def test_keys_are_the_first_leaf_of_the_restated_tree(name):
    """On small trees the restated reference tree gives the maxima and the key by the tie rule: the GPU's key is that key, or - where two
    leaves are within rounding of each other - a leaf whose restated total is the maximum."""
    from pharmaconet_amd.constants import weights_vector
    from pharmaconet_amd.engine import explain

    model, lib, weights, d = load_golden(name)
    w7 = weights_vector(weights)
    idx = [int(i) for i in np.argsort(d["n_tree"], kind="stable") if d["n_tree"][i] <= 2000][:12]
    ex = explain(model, lib, idx, weights=weights)
    exact = 0
    for r, i in enumerate(idx):
        rec = lib.unpack(i)
        T = Tables(model, rec, w7)
        lv, leaves = tree_leaves(model, rec, w7, T)
        best, keys = first_max_key(leaves, T.C)
        assert ex.levels[r].tolist() == lv
        assert np.allclose(ex.conf_max[r], best, rtol=2e-6, atol=0)
        for c in range(T.C):
            got = tuple(int(m) for m in ex.match[r][c])
            if keys[c] is None:
                assert all(m == -1 for m in got)
            elif got == keys[c]:
                exact += 1
            else:
                assert abs(path_score(model, rec, w7, lv, got, c, T) - best[c]) <= 2e-6 * best[c]
    assert exact > 0


@pytest.mark.parametrize("which", ("bench", "survey"))
def test_consistent_with_the_score_pass_on_4096_ligands(which):
    """4096 ligands of the bench library's generator / the survey library: the means are pmx_score_f64's to 4 ulp, including ligands
    whose trees the score pass splits into queued subtrees (last_score_stats()['n_tasks'] > 0 on the same slice)."""
    from pharmaconet_amd import PackedLibrary
    from pharmaconet_amd.engine import last_score_stats, screen

    model, _, _, _ = load_golden("set_6oim_c8")
    if which == "bench":
        from test_survey_library import _model_nodes
        from tools.synthetic import synthetic_library

        lib = synthetic_library(4096, model_nodes=_model_nodes(model))
    else:
        from test_survey_library import _model_nodes
        from tools.survey_library import survey_library

        centers, types = _model_nodes(model)
        off, data, _ = survey_library(centers, types, 4096, 8, "cpu")
        lib = PackedLibrary(off.numpy().astype(np.uint64), data.numpy())
    screen(model, lib, float64=True)
    stats = last_score_stats()
    assert stats["n_tasks"] > 0 or stats["n_heavy"] > 0  # the slice holds trees the score pass splits
    ex = check_against_score_pass(model, lib, None, np.arange(len(lib)), n_path=48)
    assert (ex.status == 0).all()


def test_invariance_and_two_streams(monkeypatch):
    import threading

    import torch

    from pharmaconet_amd.engine import DeviceLibrary, explain, last_score_stats, screen

    model, lib, weights, _ = load_golden("set_c21_c8")
    dlib = DeviceLibrary(lib)
    base = explain(model, dlib, np.arange(len(lib)), weights=weights)

    def same(ex, rows):
        for r, i in enumerate(rows):
            assert np.array_equal(ex.conf_max[r], base.conf_max[i]) and np.array_equal(ex.match[r], base.match[i])
            assert np.array_equal(ex.levels[r], base.levels[i]) and ex.best_conformer[r] == base.best_conformer[i]
            assert ex.status[r] == base.status[i]

    # the overflow passes: tables that do not fit an 8 KB slice, then also large slices of 1 MB (as test_gpu_api.py cuts the score pass)
    for env in ({"PMX_SLICE_KB": "8"}, {"PMX_SLICE_KB": "8", "PMX_BIG_SLICE_MB": "1", "PMX_BIG_TOTAL_MB": "64"}):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            same(explain(model, dlib, np.arange(len(lib)), weights=weights), np.arange(len(lib)))
            screen(model, dlib, weights=weights, float64=True)
            assert last_score_stats()["n_slice_overflow"] > 0, env  # the setting does reach the overflow passes

    rng = np.random.default_rng(3)
    perm = rng.permutation(len(lib))
    same(explain(model, dlib, perm, weights=weights), perm)
    sub = perm[:17]
    same(explain(model, dlib, sub, weights=weights), sub)
    rep = np.concatenate([sub, sub[::-1], sub[:3]])
    same(explain(model, dlib, rep, weights=weights), rep)
    out = {}

    def run(k):
        with torch.cuda.stream(torch.cuda.Stream()):
            out[k] = explain(model, dlib, perm, weights=weights)

    ts = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    same(out[0], perm)
    same(out[1], perm)


def test_edge_cases():
    from pharmaconet_amd import PackedLibrary
    from pharmaconet_amd.engine import explain
    from pharmaconet_amd.library import UNSUPPORTED_RECORD, LigandFeatures, pack_ligand

    model, lib, _, _ = load_golden("set_c21_c8")
    zero = pack_ligand(LigandFeatures([6, 8], [[1], [0]], [], np.zeros((2, 4, 3), np.float32)))
    hal = pack_ligand(LigandFeatures([6, 17], [[1], [0]], [("Halogen", 1, 1)], np.ones((2, 4, 3), np.float32)))
    small = PackedLibrary.from_records([zero, hal, UNSUPPORTED_RECORD, lib.record(0)])
    ex = explain(model, small, [0, 1, 2, 3, 4])
    assert ex.status.tolist() == [0, 0, 1, 0, 1]  # (index 4 is outside the library)
    for r in (0, 1):
        assert (ex.conf_max[r] == 0).all() and len(ex.conf_max[r]) == 4 and ex.match[r].size == 0 and ex.best_conformer[r] == 0
    assert np.isnan(ex.conf_max[2]).all() and ex.best_conformer[2] == -1
    assert explain(model, small, []).indices.size == 0


def test_stress_model_64_conformers_and_scoring_detail():
    from pharmaconet_amd.engine import explain

    model, lib, weights, d = load_golden("set_s64_c64")
    idx = [int(i) for i in np.argsort(d["n_tree"], kind="stable")[:: max(1, len(lib) // 16)]]
    ex = check_against_score_pass(model, lib, weights, idx, n_path=4)
    det = model.scoring_detail(lib.record(idx[0]), weights=weights)
    assert det["max"] == float(ex.conf_max[0].max()) and np.array_equal(det["conf_max"], ex.conf_max[0])
    assert abs(det["score"] - d["score"][idx[0]]) <= 2e-6 * max(abs(d["score"][idx[0]]), 1e-30)
    assert len(det["pairs"]) == len(ex.levels[0])


def test_screening_result_explain_and_cli(tmp_path):
    from conftest import GOLDEN
    from pharmaconet_amd.engine import screen
    from pharmaconet_amd.screening import main

    model, lib, weights, d = load_golden("set_6oim_c8")
    res = model.screen(lib, topk=5)
    ex = res.explain(5)
    assert ex.indices.tolist() == [i for i, _ in res.ranking()]
    shard = screen(model, lib, topk=5, index_base=1000)  # (a shard's global indices: explain takes the library's rows)
    assert shard.explain(5).indices.tolist() == ex.indices.tolist()
    libfile = tmp_path / "lib.pmxlib"
    lib.save(libfile)
    args = ["-p", str(GOLDEN / "model_6oim_like.pm"), "-d", str(libfile)]
    main(args + ["-o", str(tmp_path / "plain.csv")])
    main(args + ["-o", str(tmp_path / "with.csv"), "--explain", "5", "--explain_out", str(tmp_path / "hits.csv")])
    assert (tmp_path / "plain.csv").read_bytes() == (tmp_path / "with.csv").read_bytes()
    rows = (tmp_path / "hits.csv").read_text().splitlines()
    assert rows[0] == "rank,path,score,best_conformer,conformer_max,matches" and len(rows) == 6
    main_rows = (tmp_path / "plain.csv").read_text().splitlines()[1:6]
    K = model.flat.num_clusters
    for r, (row, mrow) in enumerate(zip(rows[1:], main_rows)):
        f = row.split(",")
        assert int(f[0]) == r + 1 and f[1] == mrow.split(",")[0] and f[2] == mrow.split(",")[1]
        assert f[5], row  # a hit matches some clusters
        for pair in f[5].split(" "):
            lc, mc = pair.split("->")
            assert 0 <= int(lc) < lib.header(int(f[1].split("#")[-1]))[2]
            assert 0 <= int(mc.split(":")[0]) < K and mc.split(":")[1] == model.flat.cluster_type[int(mc.split(":")[0])]


def test_three_entry_points_write_their_rows_and_no_more():
    """The three C entry points on raw buffers with one sentinel row (0xA5 bytes) behind what each call owns: pmx_explain and
    pmx_explain_constrained fill [n][64] and [n][64][20] - one mode of the one walker - and pmx_explain_modes [n][3][64] and
    [n][3][64][20]; the sentinel rows stay, and the owned rows are what `explain` and `explain_modes` cut their answers from."""
    import ctypes

    import torch

    from pharmaconet_amd import _ffi
    from pharmaconet_amd.engine import DeviceLibrary, _weights_array, device_model, explain, explain_modes

    model, lib, weights, _ = load_golden("set_c21_c8")
    dlib = DeviceLibrary(lib)
    idx = np.array([5, 0, len(lib) - 1, len(lib) + 7], dtype=np.int64)  # (the last one is outside the library)
    n, L, CM = len(idx), 20, 64
    dev = torch.device("cuda", dlib.device)
    head = (device_model(model, dlib.device).handle, dlib.handle, _weights_array(weights))
    lig = torch.from_numpy(idx).to(dev)
    empty = _ffi.MatchConstraint()
    calls = (("pmx_explain", (), 1, explain(model, dlib, idx, weights=weights)),
             ("pmx_explain_constrained", (ctypes.byref(empty),), 1, explain(model, dlib, idx, weights=weights, require=[], exclude=[])),
             ("pmx_explain_modes", (None, 3), 3, explain_modes(model, dlib, idx, modes=3, weights=weights)))
    for entry, which, M, want in calls:
        row = dict(values=M * CM * 8, match=M * CM * L, levels=L, best=4, status=4)  # bytes per ligand
        buf = {k: torch.full(((n + 1) * b,), 0xA5, dtype=torch.uint8, device=dev) for k, b in row.items()}
        stream = torch.cuda.current_stream(dev)
        _ffi.check(getattr(_ffi.load(), entry)(*head, *which, lig.data_ptr(), n, buf["values"].data_ptr(), buf["match"].data_ptr(), buf["levels"].data_ptr(),
                                               buf["best"].data_ptr(), buf["status"].data_ptr(), ctypes.c_void_p(stream.cuda_stream)))
        stream.synchronize()
        raw = {k: v.cpu().numpy() for k, v in buf.items()}
        for k, b in row.items():
            assert (raw[k][n * b :] == 0xA5).all(), (entry, k)
        values = raw["values"][: n * row["values"]].view(np.float64).reshape(n, M, CM)
        match = raw["match"][: n * row["match"]].reshape(n, M, CM, L)
        levels = raw["levels"][: n * L].reshape(n, L)
        best, status = raw["best"][: n * 4].view(np.int32), raw["status"][: n * 4].view(np.int32)
        ms = want if M > 1 else None
        assert status.tolist() == want.status.tolist() == [0, 0, 0, 1] and best.tolist() == want.best_conformer.tolist(), entry
        assert np.isnan(values[3]).all() and best[3] == -1, entry
        for r in range(3):
            C, nl = lib.header(int(idx[r]))[1], len(want.levels[r])
            assert levels[r, :nl].tolist() == want.levels[r].tolist() and (levels[r, nl:] == 0xFE).all(), (entry, r)
            got_v = values[r, :, :C]
            got_k = match[r, :, :C, :nl].astype(np.int64)
            got_k[got_k == 0xFF] = -1
            if ms is not None:
                assert np.array_equal(got_v, ms.values[r]) and np.array_equal(got_k, ms.match[r]), (entry, r)
            else:
                assert np.array_equal(got_v[0], want.conf_max[r]) and np.array_equal(got_k[0], want.match[r]), (entry, r)
            assert (values[r, :, C:] == 0).all() and (match[r, :, C:] == 0xFF).all() and (match[r, :, :, nl:] == 0xFF).all(), (entry, r)
