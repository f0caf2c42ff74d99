"""`pmx_library_fingerprints` and `pmx_fingerprint_search` on the GPU (csrc/pmx_ligand_fp.hip) and what the engine builds on them, against the
NumPy restatement of tests/ligand_fp_ref.py (which tests/test_ligand_fp_cpu.py holds to the header). Bits, counts and one float32 division:
every comparison here is exact."""

import ctypes
from functools import lru_cache

import numpy as np
import pytest

import ligand_fp_ref as ref
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu


def device_library(packed):
    from pharmaconet_amd.engine import DeviceLibrary

    return DeviceLibrary(packed)


def gpu_fingerprints(dlib, **kw):
    fp, tc, st = dlib.fingerprints(**kw).numpy()
    assert fp.dtype == np.uint64 and tc.dtype == np.uint8 and st.dtype == np.int32
    return fp, tc, st


def same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


@lru_cache(maxsize=None)
def fixture(name):
    """(the fixture's library with two header-only records behind it, the reference's answer for it). Made once, never written to."""
    from pharmaconet_amd.library import UNSUPPORTED_RECORD, PackedLibrary

    _, lib, _, _ = load_golden(name)
    packed = PackedLibrary.from_records([lib.record(i) for i in range(len(lib))] + [UNSUPPORTED_RECORD] * 2)
    return packed, ref.library_fingerprints(packed)


def random_record(rng, n, c, full_masks=False):
    masks = rng.integers(1, 128, n) if full_masks else (1 << rng.integers(0, 7, n)) | np.where(rng.random(n) < 0.3, 1 << rng.integers(0, 7, n), 0)
    return ref.make_record(masks, rng.uniform(-7.0, 7.0, (n, c, 3)).astype(np.float32))


@lru_cache(maxsize=None)
def hand_made():
    """Records at the definition's edges and the format's: (library, reference)."""
    from pharmaconet_amd.library import UNSUPPORTED_RECORD, PackedLibrary

    rng = np.random.default_rng(20250322)
    two = lambda x, ma=1, mb=1: ref.make_record([ma, mb], [[[0, 0, 0]], [[x, 0, 0]]])
    records = []
    for edge in (2.0, 3.0, 4.0, 5.0, 6.0, 7.5, 9.0, 12.0):
        records += [two(edge), two(float(np.nextafter(np.float32(edge), np.float32(0))))]
    records += [two(6.5, 0x7F, 0x7F), two(3.5, 1 << 2, 1 << 5), two(3.5, 1 << 5, 1 << 2), two(20.0, 1 << 6, 1 << 6), two(float("nan"))]
    records += [two(1.0, 0, 1), ref.make_record([], np.zeros((0, 1, 3))), ref.make_record([8], [[[1, 2, 3]]])]
    records += [ref.make_record([2, 32], [[[0, 0, 0], [0, 0, 0]], [[2.5, 0, 0], [0, 8, 0]]])]  # two conformers in two bins
    records += [ref.make_record([1, 1], [[[0, 0, 0]], [[1, 1, float(np.float32(np.sqrt(np.float32(2.0))))]]])]  # float32 rounds d2 to 4, float64 would not
    records += [random_record(rng, 64, 64, full_masks=True), random_record(rng, 64, 64), random_record(rng, 2, 64), random_record(rng, 64, 1),
                random_record(rng, 17, 5), random_record(rng, 33, 33), random_record(rng, 9, 3), UNSUPPORTED_RECORD]
    packed = PackedLibrary.from_records(records)
    return packed, ref.library_fingerprints(packed)


# ------------------------------------------------------------------------------------------------------------ fingerprints
@pytest.mark.parametrize("name", ("set_6oim_c1", "set_6oim_c8", "set_6oim_c64", "set_s64_c64"))
def test_fixture_libraries(name):
    packed, want = fixture(name)
    dlib = device_library(packed)
    got = gpu_fingerprints(dlib)
    assert same(got, want)
    assert got[2][-2:].tolist() == [1, 1] and (got[2][:-2] == 0).all() and not got[0][-2:].any() and not got[1][-2:].any()
    assert got[0].any() and not (got[0][:, 3] >> np.uint64(60)).any()  # bits 252 .. 255 stay 0
    first, count = 5, len(packed) - 7
    assert same(gpu_fingerprints(dlib, first=first, count=count), [w[first : first + count] for w in want])
    assert same(gpu_fingerprints(dlib, first=len(packed) - 1, count=1), [w[-1:] for w in want])
    assert len(dlib.fingerprints(first=3, count=0)) == 0
    assert dlib.fingerprints() is dlib.fingerprints()  # the union of the whole library is kept ...
    dlib.close()
    assert dlib._fingerprints is None  # ... until close


def test_hand_made_library():
    packed, want = hand_made()
    got = gpu_fingerprints(device_library(packed))
    for i in range(len(packed)):
        assert same([g[i] for g in got], [w[i] for w in want]), (i, packed.header(i))
    bits = ref.words_to_bits(got[0])
    assert [np.flatnonzero(b).tolist() for b in bits[:16]] == [[k // 2 + 1 - k % 2] for k in range(16)]  # each edge and the float below it
    assert np.flatnonzero(bits[16]).tolist() == [p * 9 + 5 for p in range(28)] and np.array_equal(bits[17], bits[18]) and np.flatnonzero(bits[19]).tolist() == [251]
    assert np.flatnonzero(bits[20]).tolist() == [0] and not bits[21:24].any() and got[2][:24].tolist() == [0] * 24
    assert got[1][21].tolist() == [1, 0, 0, 0, 0, 0, 0, 2] and got[1][22].tolist() == [0] * 8 and got[1][23].tolist() == [0, 0, 0, 1, 0, 0, 0, 1]
    assert np.flatnonzero(bits[24]).tolist() == [ref.pair_index(1, 5) * 9 + 1, ref.pair_index(1, 5) * 9 + 6] and np.flatnonzero(bits[25]).tolist() == [1]
    assert bits[26][:252].all()  # 64 nodes of random full-ish masks over 64 conformers: 2016 pairs reach every bit there is
    assert got[1][26][7] == 64 and got[2][-1] == 1


def test_conformer_keys():
    from pharmaconet_amd.library import PackedLibrary

    packed, _ = fixture("set_6oim_c8")
    hand, _ = hand_made()
    lib = PackedLibrary.from_records([packed.record(i) for i in range(40)] + [hand.record(i) for i in range(24, len(hand))] + [packed.record(len(packed) - 1)])
    dlib = device_library(lib)
    n, conf = len(lib), lib.headers()[:, 1].astype(np.int64)
    rng = np.random.default_rng(5)
    keys = np.where(conf > 0, rng.integers(0, np.maximum(conf, 1)), 0).astype(np.int32)
    keys[::4] = -1
    keys[1::8] = conf[1::8]  # C itself: no conformer of the ligand
    keys[2::8] = -2
    keys[3] = 64
    want = ref.library_fingerprints(lib, conformers=keys)
    got = gpu_fingerprints(dlib, conformers=keys)
    assert same(got, want)
    bad = ((keys < -1) | (keys >= conf)) & (conf > 0)
    assert bad.sum() >= 8 and (got[2][bad] == 4).all() and (got[2][~bad & (conf > 0)] == 0).all() and got[2][conf == 0].tolist() == [1, 1]
    assert not got[0][bad].any() and np.array_equal(got[1][bad], want[1][bad]) and got[1][bad][:, 7].all()  # no bits, but the census
    import torch

    on_device = gpu_fingerprints(dlib, conformers=torch.from_numpy(keys).cuda())
    assert same(on_device, got)
    # the union is the OR of the single conformers
    union = gpu_fingerprints(dlib)
    assert same(union, gpu_fingerprints(dlib, conformers=np.full(n, -1))) and same(union, ref.library_fingerprints(lib))
    acc = np.zeros_like(union[0])
    for c in range(int(conf.max())):
        fp, _, st = gpu_fingerprints(dlib, conformers=np.full(n, c))
        assert (st[conf > 0] == np.where(c < conf[conf > 0], 0, 4)).all() and not fp[st != 0].any()
        acc |= fp
    assert np.array_equal(acc, union[0])
    with pytest.raises(ValueError):
        dlib.fingerprints(conformers=keys[:-1])


def test_library_of_device_origin():
    packed, want = fixture("set_6oim_c8")
    dlib = device_library(packed)
    idx = np.concatenate([np.random.default_rng(9).permutation(len(packed))[:90], [len(packed) - 1, 7, 7]])
    sub = dlib.select(idx)
    assert same(gpu_fingerprints(sub), [w[idx] for w in want])
    assert same(gpu_fingerprints(sub, first=10, count=50), [w[idx[10:60]] for w in want])


def test_refusals_of_the_fingerprint_call():
    import torch

    from pharmaconet_amd import _ffi

    packed, _ = fixture("set_6oim_c1")
    dlib = device_library(packed)
    lib, n = _ffi.load(), len(packed)
    out = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for first, count in ((0, n + 1), (n, 1), (n + 1, 0), (1, 2**64 - 1)):
        assert lib.pmx_library_fingerprints(dlib.handle, first, count, None, out.data_ptr(), None, None, stream) == 1
    assert lib.pmx_library_fingerprints(None, 0, 0, None, out.data_ptr(), None, None, stream) == 1
    assert lib.pmx_library_fingerprints(dlib.handle, 0, n, None, None, None, None, stream) == 1
    assert lib.pmx_library_fingerprints(dlib.handle, n, 0, None, None, None, None, stream) == 0  # count == 0 succeeds
    assert lib.pmx_library_fingerprints(dlib.handle, 0, n, None, out.data_ptr(), None, None, stream) == 0  # counts and status are optional
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), fixture("set_6oim_c1")[1][0])
    with pytest.raises(IndexError):
        dlib.fingerprints(first=1, count=n)


# ------------------------------------------------------------------------------------------------------------------ search
@lru_cache(maxsize=None)
def noisy_prototypes():
    """5000 fingerprints around 40 prototypes of about 20 bits, each bit of a copy flipped with probability 1 %; every tenth row an exact
    copy of its prototype, some rows empty. Made once, never written to."""
    rng = np.random.default_rng(7)
    proto = rng.random((40, 256)) < 0.08
    pick = rng.integers(0, 40, 5000)
    bits = proto[pick] ^ (rng.random((5000, 256)) < 0.01)
    bits[::10] = proto[pick[::10]]
    bits[[0, 77, 4999]] = False
    return ref.bits_to_words(bits), ref.bits_to_words(proto)


def gpu_search(query, fp, stride=None, fused=True):
    """(return code, out [nq, n], fused [n]) of one `pmx_fingerprint_search`; `stride` floats per row of the output buffer."""
    import torch

    from pharmaconet_amd import _ffi

    nq, n = len(query), len(fp)
    stride = n if stride is None else stride
    tq = torch.from_numpy(np.ascontiguousarray(query).view(np.int64).reshape(-1, 4).copy()).cuda()
    tf = torch.from_numpy(np.ascontiguousarray(fp).view(np.int64).reshape(-1, 4).copy()).cuda()
    out = torch.full((max(nq, 1), max(stride, 1)), -7.0, dtype=torch.float32, device="cuda")
    fz = torch.full((max(n, 1),), -7.0, dtype=torch.float32, device="cuda")
    rc = _ffi.load().pmx_fingerprint_search(tq.data_ptr(), nq, tf.data_ptr(), n, out.data_ptr(), stride, fz.data_ptr() if fused else None, 0,
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), fz.cpu().numpy()[:n]


@pytest.mark.parametrize("nq", (1, 3, 64))
def test_search_matches_numpy(nq):
    fp, proto = noisy_prototypes()
    query = np.concatenate([np.zeros((1, 4), dtype=np.uint64), proto, fp[100:123]])[:nq] if nq > 1 else proto[:1]
    want_out, want_fused = ref.search(query, fp)
    rc, out, fused = gpu_search(query, fp)
    assert rc == 0 and np.array_equal(out.view(np.uint32), want_out.view(np.uint32)) and np.array_equal(fused.view(np.uint32), want_fused.view(np.uint32))
    if nq > 1:
        assert out[0, 0] == 1.0 and out[0, 77] == 1.0 and out[0, 1] == 0.0  # two empty sets
    rc, wide, fused2 = gpu_search(query, fp, stride=len(fp) + 37)
    assert rc == 0 and np.array_equal(wide[:, : len(fp)], out) and (wide[:, len(fp) :] == -7.0).all() and np.array_equal(fused2, fused)
    rc, out3, untouched = gpu_search(query, fp[:257], fused=False)  # one row past a block, no fused column
    assert rc == 0 and np.array_equal(out3, out[:, :257]) and (untouched == -7.0).all()


def test_search_refusals():
    from pharmaconet_amd import _ffi

    fp, proto = noisy_prototypes()
    assert gpu_search(proto[:0], fp[:10])[0] == 1 and b"queries" in _ffi.load().pmx_last_error()
    assert gpu_search(np.concatenate([proto, proto])[:65], fp[:10])[0] == 1
    assert gpu_search(proto[:2], fp[:10], stride=9)[0] == 1 and b"out_stride" in _ffi.load().pmx_last_error()
    rc, out, _ = gpu_search(proto[:2], fp[:0])  # n = 0 succeeds and writes nothing
    assert rc == 0 and (out == -7.0).all()
    assert gpu_search(proto[:2], fp[:10])[0] == 0  # (and the next call is served)


# ------------------------------------------------------------------------------------------------------------------ engine
@pytest.fixture(scope="module")
def golden_screen():
    model, lib, weights, _ = load_golden("set_6oim_c8")
    dlib = device_library(lib)
    return model, lib, dlib, weights, model.screen(dlib, weights=weights), ref.library_fingerprints(lib)


def stable_descending(values, k):
    return np.lexsort((np.arange(len(values)), -values.astype(np.float64)))[:k]


def test_similar_by_query_indices(golden_screen):
    from pharmaconet_amd import engine

    _, lib, dlib, _, _, (fp, _, st) = golden_screen
    qidx = np.array([3, 50, 200])
    want_out, want_fused = ref.search(fp[qidx], fp)
    res = engine.similar(dlib, query_indices=qidx, k=25)
    out, fused = res.scores.cpu().numpy(), res.fused.cpu().numpy()
    assert tuple(out.shape) == (3, len(lib)) and np.array_equal(out.view(np.uint32), want_out.view(np.uint32)) and np.array_equal(fused.view(np.uint32), want_fused.view(np.uint32))
    order = stable_descending(want_fused, 25)
    assert np.array_equal(res.topk_indices.cpu().numpy(), order) and np.array_equal(res.topk_scores.cpu().numpy(), want_fused[order])
    assert [i for i, _ in res.ranking()] == order.tolist() and np.array_equal(res.status.cpu().numpy(), st)
    for q, i in enumerate(qidx):  # a query is 1.0 similar to itself: nothing in its column is above it
        assert out[q, i] == 1.0 and out[q].max() == 1.0 and fused[i] == 1.0
    # the same queries as a library of their own, on the host or resident
    for queries in (lib.select(qidx), dlib.select(qidx)):
        again = engine.similar(dlib, queries=queries, k=None)
        assert again.topk_indices is None and again.query_indices is None and np.array_equal(again.scores.cpu().numpy(), out)
    assert np.array_equal(engine.similar(lib, query_indices=qidx, k=None).fused.cpu().numpy(), fused)  # a host library is uploaded for the call
    # queries as posed: one conformer each
    conf = [2, -1, 7]
    posed = engine.similar(dlib, query_indices=qidx, query_conformers=conf, k=None)
    qfp = ref.library_fingerprints(lib.select(qidx), conformers=conf)[0]
    assert np.array_equal(posed.scores.cpu().numpy().view(np.uint32), ref.search(qfp, fp)[0].view(np.uint32))
    for kw in (dict(), dict(queries=lib.select(qidx), query_indices=qidx), dict(query_indices=[len(lib)]), dict(query_indices=np.arange(65)), dict(query_indices=[])):
        with pytest.raises((ValueError, IndexError)):
            engine.similar(dlib, k=None, **kw)


def test_similarity_enrichment(golden_screen):
    import torch

    from pharmaconet_amd import engine

    _, lib, dlib, _, _, _ = golden_screen
    labels = (np.random.default_rng(11).random(len(lib)) < 0.2).astype(np.uint8)
    qidx = np.flatnonzero(labels)[:2]
    res = engine.similar(dlib, query_indices=qidx)
    en = res.enrichment(labels, bootstrap=4, seed=3)
    relabelled = labels.copy()
    relabelled[qidx] = 2
    want = engine.enrichment(torch.cat([res.scores, res.fused[None]]), relabelled, status=res.status, bootstrap=4, seed=3)
    assert en.columns == [0, 1, "fused"] and en.n_active == int(labels.sum()) - 2 and labels[qidx].tolist() == [1, 1]
    assert (en.totals == want.totals).all() and (en.u2 == want.u2).all()
    assert (en.hits.view(np.uint64) == want.hits.view(np.uint64)).all() and (en.expsum.view(np.uint64) == want.expsum.view(np.uint64)).all()
    assert en.auroc.tolist() == want.auroc.tolist() and en.delta("fused", 0, "auroc")["value"] == en.auroc[2] - en.auroc[0]
    on_device = res.enrichment(torch.from_numpy(labels).cuda(), bootstrap=4, seed=3)
    assert (on_device.u2 == en.u2).all()


def test_similar_to_a_hit_as_posed(golden_screen):
    _, lib, dlib, _, result, (fp, _, _) = golden_screen
    ex = result.explain(2)
    hit, conformer = int(ex.indices[1]), int(ex.best_conformer[1])
    res = result.similar_to(1, k=10)
    posed = ref.bits_to_words(ref.record_fingerprint(lib.unpack(hit), conformer)[0])
    want_out, want_fused = ref.search(posed[None], fp)
    assert res.query_indices.tolist() == [hit] and np.array_equal(res.scores.cpu().numpy().view(np.uint32), want_out.view(np.uint32))
    assert np.array_equal(res.topk_indices.cpu().numpy(), stable_descending(want_fused, 10))
    with pytest.raises(IndexError):
        result.similar_to(len(lib))


def test_diverse_ligands(golden_screen):
    from pharmaconet_amd.engine import DiverseHits

    _, lib, dlib, _, result, (fp, _, _) = golden_screen
    scores, status = result.scores.cpu().numpy(), result.status.cpu().numpy()
    assert (status == 0).all()
    for k, pool, threshold in ((10, 100, 0.4), (5, None, 0.3), (300, 304, 0.7)):
        dv = result.diverse_ligands(k, pool=pool, threshold=threshold)
        ranked = stable_descending(scores, len(lib) if pool is None else pool)  # (pool None: min(len, max(8 k, 1024), 65536) is the whole list here)
        want_lead, want_of = ref.leaders(fp[ranked], threshold, min(k, 2048))
        assert isinstance(dv, DiverseHits) and dv.profile is None and len(dv) == len(want_lead) <= k
        assert np.array_equal(dv.leaders, want_lead) and np.array_equal(dv.leader_of, want_of) and np.array_equal(dv.pool, ranked)
        assert np.array_equal(dv.indices, ranked[want_lead]) and np.array_equal(dv.scores, scores[ranked[want_lead]].astype(np.float64))
        assert np.array_equal(dv.cluster_size, np.bincount(want_of[want_of >= 0], minlength=len(ranked))[want_lead])
    assert (dv.cluster_size >= 1).all()
    with pytest.raises(ValueError):
        result.diverse_ligands(0)


def test_where_filters_by_the_census():
    import torch

    packed, (_, tc, st) = fixture("set_6oim_c8")
    dlib = device_library(packed)
    tc = tc.astype(np.int64)
    got = dlib.where(min_counts={"Aromatic": 2, "HBond_acceptor": 1}, max_counts={"Cation": 0}, max_nodes=20)
    want = np.flatnonzero((st == 0) & (tc[:, 1] >= 2) & (tc[:, 5] >= 1) & (tc[:, 2] <= 0) & (tc[:, 7] <= 20))
    assert got.dtype == torch.int64 and got.is_cuda and 0 < len(want) < len(packed) - 2 and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(dlib.where(min_counts=[0, 1, 0, 0, 2, 0, 0]).cpu().numpy(), np.flatnonzero((st == 0) & (tc[:, 1] >= 1) & (tc[:, 4] >= 2)))
    assert np.array_equal(dlib.where().cpu().numpy(), np.arange(len(packed) - 2))  # everything but the two header-only records
    assert np.array_equal(dlib.where(max_nodes=0).cpu().numpy(), np.flatnonzero((st == 0) & (tc[:, 7] == 0)))  # (a record may have no node and be supported)
    assert len(dlib.where(max_counts=[0] * 7, min_counts={"Halogen": 1})) == 0
    sub = dlib.select(got)
    assert len(sub) == len(want) and np.array_equal(sub.fingerprints().numpy()[1].astype(np.int64), tc[want])
    with pytest.raises(ValueError):
        dlib.where(min_counts={"Aromatics": 1})


def test_fingerprint_rows_compare_and_cluster():
    packed, (fp, _, _) = fixture("set_6oim_c64")
    fps = device_library(packed).fingerprints()
    sim = fps.similarity()
    assert np.array_equal(sim.view(np.uint32), ref.search(fp, fp)[0].view(np.uint32)) and sim[-1, -2] == 1.0  # (the two empty rows)
    lead, of = fps.leaders(threshold=0.35)
    want_lead, want_of = ref.leaders(fp, 0.35, 2048)
    assert np.array_equal(lead, want_lead) and np.array_equal(of, want_of)


# --------------------------------------------------------------------------------------------------------------------- CLI
def test_cli_similar_out(tmp_path, golden_screen):
    from pharmaconet_amd.screening import main

    _, lib, _, _, _, (fp, _, _) = golden_screen
    libfile = tmp_path / "lib.pmxlib"
    lib.save(libfile)
    (tmp_path / "lib.pmxlib.names").write_text("\n".join(f"/data/mol_{i}.sdf" for i in range(len(lib))))
    base = ["-p", str(GOLDEN / "model_6oim_like.pm"), "-d", str(libfile)]
    main(base + ["-o", str(tmp_path / "plain.csv")])
    main(base + ["-o", str(tmp_path / "out.csv"), "--similar_to", "mol_12", "--similar_to", "/data/mol_150.sdf", "--similar_out", str(tmp_path / "s.csv"), "--similar_k", "15"])
    assert (tmp_path / "out.csv").read_bytes() == (tmp_path / "plain.csv").read_bytes()
    want_out, want_fused = ref.search(fp[[12, 150]], fp)
    rows = [ln.split(",") for ln in (tmp_path / "s.csv").read_text().splitlines()]
    assert rows[0] == ["rank", "path", "similarity", "mol_12", "mol_150"] and len(rows) == 16
    for r, i in enumerate(stable_descending(want_fused, 15)):
        assert rows[r + 1] == [str(r + 1), f"/data/mol_{i}.sdf", str(float(want_fused[i])), str(float(want_out[0, i])), str(float(want_out[1, i]))]
    assert {rows[1][1], rows[2][1]} == {"/data/mol_12.sdf", "/data/mol_150.sdf"} and rows[1][2] == "1.0"
    for bad in (["--similar_to", "mol_12"], ["--similar_out", str(tmp_path / "x.csv")], ["--similar_to", "mol_999999", "--similar_out", str(tmp_path / "x.csv")],
                ["--similar_to", "mol_12", "--similar_to", "mol_12", "--similar_out", str(tmp_path / "x.csv")]):
        with pytest.raises(SystemExit):
            main(base + ["-o", str(tmp_path / "err.csv")] + bad)
