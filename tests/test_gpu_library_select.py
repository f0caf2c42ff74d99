"""Sub-libraries on the device: `pmx_library_select` (csrc/pmx_select.hip) and what is built on it - `DeviceLibrary.select` / `download`, listed
screens, `screen_multi`, `ScreeningResult.panel` and the CLI's `--panel` / `--save_top`. The yardstick of the gather is the host gather
(`PackedLibrary.select`, tests/test_library_select_cpu.py), byte for byte; the yardstick of a listed score is the same ligand's score in
the whole library, bit for bit."""

import ctypes
import functools

import numpy as np
import pytest

from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

BIG = 49296  # bytes of a 64-node, 64-cluster, 64-conformer record: the largest the format has


def same(a, b):
    return np.array_equal(a.offsets.astype(np.uint64), b.offsets.astype(np.uint64)) and a.data.size == b.data.size and np.array_equal(a.data, b.data)


def info(dlib):
    return (dlib.num_ligands, dlib.num_bytes, dlib.total_conformers, dlib.max_nodes, dlib.max_conformers, dlib.max_clusters, dlib.num_unsupported)


@functools.lru_cache(maxsize=None)
def with_markers(name):
    """The fixture's library with two header-only records appended, on the host and resident."""
    from pharmaconet_amd import PackedLibrary
    from pharmaconet_amd.engine import DeviceLibrary
    from pharmaconet_amd.library import UNSUPPORTED_RECORD

    lib = load_golden(name)[1]
    host = PackedLibrary.from_records([lib.record(i) for i in range(len(lib))] + [UNSUPPORTED_RECORD] * 2)
    return host, DeviceLibrary(host)


def lists(n, seed):
    rng = np.random.default_rng(seed)
    return {"permutation with repeats": np.concatenate([rng.permutation(n), rng.integers(0, n, n // 2 + 3)]), "reversed": np.arange(n)[::-1].copy(), "empty": np.zeros(0, np.int64)}


def check_selection(host, dlib, idx):
    from pharmaconet_amd.engine import DeviceLibrary

    want = host.select(idx)
    sel = dlib.select(idx)
    assert same(sel.download(), want)
    up = DeviceLibrary(want)
    assert info(sel) == info(up)
    sel.close()
    up.close()


@pytest.mark.parametrize("name", ["set_6oim_c1", "set_6oim_c8", "set_6oim_c64", "set_s64_c64"])
def test_select_then_download_is_the_host_selection(name):
    host, dlib = with_markers(name)
    for what, idx in lists(len(host), 17).items():
        check_selection(host, dlib, idx)
    assert same(dlib.download(), host)  # (a library uploaded from the host, read back through pmx_library_buffers)


def test_select_takes_a_list_an_array_and_a_device_tensor():
    import torch

    host, dlib = with_markers("set_6oim_c8")
    idx = lists(len(host), 2)["permutation with repeats"]
    want = host.select(idx)
    on_device = torch.from_numpy(idx).cuda()
    for form in (idx.tolist(), idx, idx.astype(np.int32), on_device):
        sel = dlib.select(form)
        assert same(sel.download(), want)
        sel.close()
    with pytest.raises(TypeError):
        dlib.select(on_device.to(torch.int32))
    with pytest.raises(IndexError):
        dlib.select([0, -1])


def test_select_from_libraries_of_every_origin():
    """Packed on the device and adopted (`from_features`), copied on the device (`from_device_buffers(adopt=False)`: a library that kept nothing
    but its handle), and a selection itself."""
    import torch

    from pharmaconet_amd.engine import DeviceLibrary, explain
    from pharmaconet_amd.library import flatten_features
    from test_library import golden_molecules

    model, host, weights, _ = load_golden("set_6oim_c8")
    idx = lists(len(host), 23)["permutation with repeats"]
    made = DeviceLibrary.from_features(flatten_features(list(golden_molecules("set_6oim_c8"))))
    copied = DeviceLibrary.from_device_buffers(torch.from_numpy(host.offsets.astype(np.int64)).cuda(), torch.from_numpy(np.ascontiguousarray(host.data)).cuda(), adopt=False)
    for dlib in (made, copied):
        assert same(dlib.download(), host)
        check_selection(host, dlib, idx)
    first = copied.select(idx)
    again = np.random.default_rng(4).integers(0, len(idx), 100)
    check_selection(host.select(idx), first, again)
    # a library that kept no record sizes is explained through its buffers, and a selection like any adopted library
    want = explain(model, host, idx[:5], weights=weights)
    for dlib, rows in ((copied, idx[:5]), (first, np.arange(5))):
        got = explain(model, dlib, rows, weights=weights)
        assert all(np.array_equal(a, b) for a, b in zip(got.conf_max, want.conf_max)) and all(np.array_equal(a, b) for a, b in zip(got.match, want.match))
    for dlib in (made, copied, first):
        dlib.close()


@functools.lru_cache(maxsize=None)
def mixed_sizes():
    """Records of 16, 32, 1024, 1040 and 49 296 bytes, every size next to every other: the sizes at which the copy's trips begin and end."""
    from pharmaconet_amd import PackedLibrary
    from pharmaconet_amd.engine import DeviceLibrary
    from pharmaconet_amd.library import UNSUPPORTED_RECORD, ClusteredLigand, pack_clustered_ligand

    rng = np.random.default_rng(8)

    def record(n, conformers, clusters):
        cl = ClusteredLigand(rng.integers(1, 128, n).astype(np.uint8), rng.normal(size=(n, conformers, 3)).astype(np.float32), clusters, ["Hydrophobic"] * len(clusters),
                             list(range(len(clusters))))
        return pack_clustered_ligand(cl)

    kinds = [UNSUPPORTED_RECORD, record(1, 1, [[0]]), record(7, 12, [list(range(7))]), record(7, 12, [list(range(6)), [6]]), record(64, 64, [[i] for i in range(64)])]
    assert [len(k) for k in kinds] == [16, 32, 1024, 1040, BIG]
    order = [a for i in range(5) for j in range(5) for a in (i, j)]  # every ordered pair of sizes as neighbours
    host = PackedLibrary.from_records([kinds[k] for k in order])
    return host, DeviceLibrary(host), order


@pytest.mark.parametrize("length", [1, 63, 64, 65, 257])
def test_select_of_mixed_record_sizes(length):
    host, dlib, order = mixed_sizes()
    rng = np.random.default_rng(length)
    idx = rng.integers(0, len(host), length)
    idx[0] = order.index(4)  # (the largest record is always there; from two on, the smallest ends the list)
    if length > 1:
        idx[-1] = order.index(0)
    sel = dlib.select(idx)
    assert same(sel.download(), host.select(idx))
    sel.close()


def test_select_beyond_four_gib():
    """The largest record listed 90 000 times: 4.44 x 10^9 bytes, offsets and copy positions beyond 2^32."""
    import torch

    free, _ = torch.cuda.mem_get_info()
    if free < 12e9:
        pytest.skip("less than 12 GB of device memory free")
    host, dlib, order = mixed_sizes()
    big = order.index(4)
    n = 90_000
    sel = dlib.select(torch.full((n,), big, dtype=torch.int64, device="cuda"))
    offsets, data = sel.buffers()
    assert sel.num_bytes == n * BIG and data.numel() == n * BIG
    assert bool((offsets == torch.arange(n + 1, dtype=torch.int64, device="cuda") * BIG).all())
    want = np.frombuffer(host.record(big), dtype=np.uint8)
    for i in (0, 87_127, 87_128, 87_130, n - 1):  # 87 127 straddles 2^32, the others lie beyond it
        assert np.array_equal(data[i * BIG : (i + 1) * BIG].cpu().numpy(), want), i
    sel.close()
    del offsets, data
    torch.cuda.empty_cache()


def test_select_errors_leave_the_output_alone():
    """include/pmx.h: an index outside the library fails the call and names its position, a data_cap that is too small fails it with the need;
    neither writes a record. The sizing call writes offsets only."""
    import torch

    from pharmaconet_amd import _ffi

    host, dlib = with_markers("set_6oim_c8")
    lib = _ffi.load()
    n_lig = len(host)
    good = np.array([5, 0, n_lig - 1, 7, 7, 2], dtype=np.int64)
    want = host.select(good)
    offsets = torch.zeros(len(good) + 1, dtype=torch.int64, device="cuda")
    data = torch.full((want.data.size + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    nbytes = ctypes.c_uint64(0)

    def call(idx, out, cap):
        t = torch.from_numpy(np.asarray(idx, dtype=np.int64)).cuda()
        rc = lib.pmx_library_select(dlib.handle, t.data_ptr(), len(idx), offsets.data_ptr(), out, cap, ctypes.byref(nbytes), None)
        torch.cuda.synchronize()
        return rc

    untouched = lambda: bool((data == 0xAB).all())
    # sizing alone
    assert call(good, None, 0) == 0 and int(nbytes.value) == want.data.size and untouched()
    assert np.array_equal(offsets.cpu().numpy().astype(np.uint64), want.offsets)
    # one bad index among good ones, and two
    bad = good.copy()
    bad[3] = n_lig
    assert call(bad, data.data_ptr(), data.numel()) == 1 and untouched()
    msg = lib.pmx_last_error().decode()
    assert "1 of 6 indices" in msg and "position 3" in msg, msg
    bad[1] = 2**40
    assert call(bad, data.data_ptr(), data.numel()) == 1 and untouched()
    msg = lib.pmx_last_error().decode()
    assert "2 of 6 indices" in msg and "position 1" in msg, msg
    with pytest.raises(_ffi.PmxError, match="position 3"):
        dlib.select([0, 1, 2, n_lig + 1, 4])
    # too small
    assert call(good, data.data_ptr(), want.data.size - 16) == 1 and untouched()
    assert int(nbytes.value) == want.data.size and "too small" in lib.pmx_last_error().decode()
    # a sizing call must not come with a capacity; the output must not be the library itself
    assert call(good, None, 16) == 1
    lib_offsets, lib_data = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.pmx_library_buffers(dlib.handle, ctypes.byref(lib_offsets), ctypes.byref(lib_data)) == 0
    assert call(good, lib_data.value, want.data.size) == 1 and "overlaps" in lib.pmx_last_error().decode()
    # and the call that fits: exactly the records, nothing behind them
    assert call(good, data.data_ptr(), want.data.size) == 0 and int(nbytes.value) == want.data.size
    got = data.cpu().numpy()
    assert np.array_equal(got[: want.data.size], want.data) and (got[want.data.size :] == 0xAB).all()
    # no indices: an empty library
    offsets.fill_(7)
    assert call([], None, 0) == 0 and int(nbytes.value) == 0 and int(offsets[0]) == 0


def test_selects_on_two_streams_share_the_work_buffers():
    import torch

    host, dlib, _ = mixed_sizes()
    small_host, small = with_markers("set_6oim_c8")
    a = np.random.default_rng(1).integers(0, len(host), 3000)
    b = np.random.default_rng(2).integers(0, len(small_host), 500)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for _ in range(2):
        with torch.cuda.stream(streams[0]):
            sa = dlib.select(a)
        with torch.cuda.stream(streams[1]):
            sb = small.select(b)
        torch.cuda.synchronize()
        assert same(sa.download(), host.select(a)) and same(sb.download(), small_host.select(b))
        sa.close()
        sb.close()


@functools.lru_cache(maxsize=None)
def whole_screen(name, float64):
    """The fixture, resident, and its whole-library screen: computed once, read by every test below."""
    from pharmaconet_amd.engine import DeviceLibrary, screen

    model, lib, weights, _ = load_golden(name)
    dlib = DeviceLibrary(lib)
    res = screen(model, dlib, weights=weights, float64=float64)
    return model, lib, weights, dlib, res.scores.cpu().numpy(), res.status.cpu().numpy()


@pytest.mark.parametrize("float64", [False, True])
@pytest.mark.parametrize("name", ["set_6oim_c8", "set_6oim_c8_weights", "set_l110_c8"])
def test_listed_screen_scores_like_the_whole_library(name, float64):
    from pharmaconet_amd.engine import screen

    model, lib, weights, dlib, scores, status = whole_screen(name, float64)
    idx = lists(len(lib), 31)["permutation with repeats"]
    listed = screen(model, dlib, weights=weights, indices=idx, float64=float64)
    assert np.array_equal(listed.indices.cpu().numpy(), idx)
    sub = dlib.select(idx)
    of_selection = screen(model, sub, weights=weights, float64=float64)
    for got in (listed, of_selection):
        assert got.scores.dtype == listed.scores.dtype and np.array_equal(got.scores.cpu().numpy(), scores[idx], equal_nan=True)
        assert np.array_equal(got.status.cpu().numpy(), status[idx])
    sub.close()
    with pytest.raises(ValueError):
        screen(model, dlib, indices=idx, first=1)
    with pytest.raises(ValueError):
        screen(model, dlib, indices=idx, count=3)


def test_listed_screen_ranks_by_score_then_list_position():
    from pharmaconet_amd.engine import explain, screen

    model, lib, weights, dlib, scores, status = whole_screen("set_6oim_c8", False)
    idx = lists(len(lib), 37)["permutation with repeats"]  # (repeats: equal scores at different list positions)
    k = 40
    res = screen(model, dlib, weights=weights, indices=idx, topk=k)
    sc = scores[idx]
    assert len(np.unique(sc)) < len(sc)
    order = np.lexsort((np.arange(len(idx)), -sc.astype(np.float64)))[:k]
    assert np.array_equal(res.topk_indices.cpu().numpy(), idx[order]) and np.array_equal(res.topk_scores.cpu().numpy(), sc[order])
    assert len(set(sc[order].tolist())) < k  # (ties inside the ranking itself)
    shifted = screen(model, dlib, weights=weights, indices=idx, topk=k, index_base=1000)
    assert np.array_equal(shifted.topk_indices.cpu().numpy(), idx[order] + 1000)
    # explain(k) of a listed screen: those library ligands, explained against the original library - with and without a device ranking
    want = explain(model, dlib, idx[order[:3]], weights=weights)
    for r in (res, screen(model, dlib, weights=weights, indices=idx)):
        got = r.explain(3)
        assert np.array_equal(got.indices, idx[order[:3]]) and np.array_equal(got.best_conformer, want.best_conformer)
        assert all(np.array_equal(a, b) for a, b in zip(got.conf_max, want.conf_max)) and all(np.array_equal(a, b) for a, b in zip(got.match, want.match))


def test_screen_multi_and_panel():
    from pharmaconet_amd import PharmacophoreModel
    from pharmaconet_amd.engine import screen, screen_multi

    m0, lib, weights, dlib, scores, status = whole_screen("set_6oim_c8", False)
    m1 = PharmacophoreModel.load(GOLDEN / "model_clustered21.pm")
    other = screen(m1, dlib, weights=weights)
    other_scores = other.scores.cpu().numpy()
    for float64 in (False, True):
        want = [screen(m, dlib, weights=weights, float64=float64).scores.cpu().numpy() for m in (m0, m1)] if float64 else [scores, other_scores]
        panel = screen_multi([m0, m1], dlib, weights=weights, float64=float64)
        got = panel.scores.cpu().numpy()
        assert got.shape == (2, len(lib)) and got.dtype == want[0].dtype
        assert np.array_equal(got[0], want[0], equal_nan=True) and np.array_equal(got[1], want[1], equal_nan=True)
        assert np.array_equal(panel.status.cpu().numpy(), status)
    # a range, and the best of a pocket
    part = screen_multi([m0, m1], dlib, weights=weights, first=3, count=20)
    assert np.array_equal(part.scores.cpu().numpy(), np.stack([scores[3:23], other_scores[3:23]]))
    best_i, best_s = part.best(1, 4)
    order = np.lexsort((np.arange(20), -other_scores[3:23].astype(np.float64)))[:4]
    assert np.array_equal(best_i, order + 3) and np.array_equal(best_s, other_scores[3:23][order])
    # ScreeningResult.panel: the screen's k best against the other pocket
    k = 12
    res = screen(m0, dlib, weights=weights, topk=k)
    top = res.topk_indices.cpu().numpy()
    pan = res.panel(k, [m1])
    ps = pan.scores.cpu().numpy()
    assert np.array_equal(pan.indices.cpu().numpy(), top)
    assert np.array_equal(ps[0], res.topk_scores.cpu().numpy()) and np.array_equal(ps[1], other_scores[top])
    assert np.array_equal(pan.margin(0).cpu().numpy(), ps[0] - ps[1]) and np.array_equal(pan.margin(1).cpu().numpy(), ps[1] - ps[0])
    with pytest.raises(ValueError):
        screen_multi([m0], dlib).margin(0)


def test_screen_multi_and_panel_one_pocket_one_answer():
    """The bit-equalities of the test above under {"Halogen": 100}: model_clustered21 holds no Halogen, Aromatic or Anion node, so alone its
    weights are 8 : 1 apart and its pair items read the tables; model_6oim_like's are 100 : 1 apart and take the term-by-term tails. In a
    panel each pocket is still scored as `screen` scores it alone, and as `explain` explains it (means of the maxima, 4 ulp)."""
    from pharmaconet_amd import PharmacophoreModel
    from pharmaconet_amd.constants import TYPE_ID
    from pharmaconet_amd.engine import explain, screen, screen_multi

    weights = {"Halogen": 100.0}
    m0, lib, _, dlib, _, status = whole_screen("set_6oim_c8", False)
    m1 = PharmacophoreModel.load(GOLDEN / "model_clustered21.pm")
    held = [{int(t) for t in m.flat.node_type} for m in (m0, m1)]
    assert TYPE_ID["Halogen"] in held[0] and not held[1] & {TYPE_ID[t] for t in ("Halogen", "Aromatic", "Anion")}
    for float64 in (False, True):
        want = [screen(m, dlib, weights=weights, float64=float64).scores.cpu().numpy() for m in (m0, m1)]
        for models, rows in (([m0, m1], (0, 1)), ([m1, m0], (1, 0))):
            panel = screen_multi(models, dlib, weights=weights, float64=float64)
            got = panel.scores.cpu().numpy()
            assert got.shape == (2, len(lib)) and got.dtype == want[0].dtype
            for r, m in enumerate(rows):
                differ = np.flatnonzero(~((got[r] == want[m]) | (np.isnan(got[r]) & np.isnan(want[m]))))
                assert differ.size == 0, (float64, rows, m, differ[:8].tolist(), got[r][differ[:8]].tolist(), want[m][differ[:8]].tolist())
            assert np.array_equal(panel.status.cpu().numpy(), status)
    assert np.count_nonzero(want[1]) > len(lib) // 2  # (float64 columns from here on)
    # (explain walks a tree to its end with one wavefront: of model_6oim_like's, those the reference counts at most 10^5 nodes in; the others' all)
    light = np.flatnonzero(load_golden("set_6oim_c8")[3]["n_tree"] <= 100000)
    for m, column, idx in ((m0, got[1], light), (m1, got[0], np.arange(len(lib)))):  # the last panel was [m1, m0]
        ex = explain(m, dlib, idx, weights=weights)
        ok = status[idx] == 0
        assert np.array_equal(ex.status, status[idx]) and ok.sum() > len(lib) // 2
        means = np.array([v.mean() for v in ex.conf_max])[ok]
        assert (np.abs(means - column[idx][ok]) <= 4 * np.spacing(np.maximum(np.abs(means), np.abs(column[idx][ok])))).all()
    # ScreeningResult.panel: the screen's k best against the other pocket
    k = 12
    other_scores = screen(m1, dlib, weights=weights).scores.cpu().numpy()
    res = screen(m0, dlib, weights=weights, topk=k)
    top = res.topk_indices.cpu().numpy()
    ps = res.panel(k, [m1]).scores.cpu().numpy()
    assert np.array_equal(ps[0], res.topk_scores.cpu().numpy()) and np.array_equal(ps[1], other_scores[top])


def test_cli_panel_and_save_top(tmp_path):
    from pharmaconet_amd import PackedLibrary
    from pharmaconet_amd.screening import main

    _, lib, _, _ = load_golden("set_6oim_c8")
    libfile = tmp_path / "lib.pmxlib"
    lib.save(libfile)
    (tmp_path / "lib.pmxlib.names").write_text("\n".join(f"mol_{i}.sdf" for i in range(len(lib))))
    base = ["-p", str(GOLDEN / "model_6oim_like.pm"), "-d", str(libfile)]
    main(base + ["-o", str(tmp_path / "plain.csv")])
    saved = tmp_path / "top.pmxlib"
    main(base + ["-o", str(tmp_path / "out.csv"), "--panel", str(GOLDEN / "model_clustered21.pm"), "--panel", str(GOLDEN / "model_stress64.pm"), "--panel_k", "5",
                 "--panel_out", str(tmp_path / "panel.csv"), "--save_top", "5", str(saved)])
    assert (tmp_path / "out.csv").read_bytes() == (tmp_path / "plain.csv").read_bytes()
    main_rows = [ln.split(",") for ln in (tmp_path / "out.csv").read_text().splitlines()[1:6]]
    panel = [ln.split(",") for ln in (tmp_path / "panel.csv").read_text().splitlines()]
    assert panel[0] == ["rank", "path", "score", "model_clustered21", "model_stress64", "margin"] and len(panel) == 6
    for r, (row, (name, score)) in enumerate(zip(panel[1:], main_rows)):
        assert row[:3] == [str(r + 1), name, score]
        assert float(row[5]) == float(row[2]) - max(float(row[3]), float(row[4]))
    # the saved hits are a library that screens to the same five lines
    top = PackedLibrary.load(saved)
    names = (tmp_path / "top.pmxlib.names").read_text().splitlines()
    assert len(top) == 5 and names == [name for name, _ in main_rows]
    assert [top.record(i) for i in range(5)] == [lib.record(int(name[4:-4])) for name in names]
    main(["-p", str(GOLDEN / "model_6oim_like.pm"), "-d", str(saved), "-o", str(tmp_path / "again.csv")])
    assert [ln.split(",") for ln in (tmp_path / "again.csv").read_text().splitlines()[1:]] == main_rows
    for flags in (["--panel", str(GOLDEN / "model_clustered21.pm")], ["--panel_out", str(tmp_path / "x.csv")]):
        with pytest.raises(SystemExit):
            main(base + ["-o", str(tmp_path / "err.csv")] + flags)
