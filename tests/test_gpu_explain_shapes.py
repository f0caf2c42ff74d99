"""The explain family at every lane shape. `pmx_explain`, `pmx_explain_constrained` and `pmx_explain_modes` run as
explain_kernel<G, ...> with G = 2^ceil(log2(the library's most conformers)); the fixtures and synthetic libraries of test_gpu_explain.py,
test_gpu_constrained.py and test_gpu_modes.py have 1, 5, 8 or 64 conformers, so G = 2, 4, 16, 32 and the partly filled groups (C = 3, 12,
20, 33, 48) are checked here, on the libraries test_gpu_variants.py::test_every_lane_shape_matches_the_oracle scores. The reference is
`oracle_explain` (oracle/pmx_oracle.c), pinned to the reference's own leaves by tests/test_oracle_explain.py: every ligand, whatever its
tree's size. Bars: 2e-6 relative for a total and the 1e-5 gap rule for a key, as the fixture tests of the three calls have them."""

import ctypes
import functools
import os

import numpy as np
import pytest

from conftest import load_golden
from constrained_ref import qualifies, random_constraint
from explain_ref import NONE, Tables, candidates, ligand_levels, path_score
from tail_cases import PAIR_SHAPE_SETS, SHAPES, WEIGHT_SETS, _Shim, pair_shape_cases, pair_shape_explained

pytestmark = pytest.mark.gpu

RTOL = 2e-6  # test_gpu_parity.py's RTOL
TIE = 1e-5  # a key is pinned where the next total lies more than this (relative) below
CONFORMERS = [2, 3, 4, 12, 16, 20, 32, 33, 48]
LIBRARIES = (("set_6oim_c8", 160), ("set_s64_c8", 48))
MAX_MODES = 8
# type weights further apart than PMX_TAILS_RATIO: the first ligands of the same libraries, at G = 1 ... 64
SPREAD_CONFORMERS = (1, 2, 3, 8, 12, 20, 33)
SPREAD_WEIGHTS = ("charged_heavy", "charged_light")
SPREAD_LIBRARIES = (("set_6oim_c8", 64), ("set_s64_c8", 24))
THREADS = min(os.cpu_count() or 8, 16)


def _model_nodes(model):
    from pharmaconet_amd.constants import TYPE_ID

    st = model.__getstate__()
    return np.array([n["center"] for n in st["nodes"]], dtype=np.float64), np.array([TYPE_ID[n["type"]] for n in st["nodes"]])


def ulp_close(a, b, n=4):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) <= n * np.spacing(np.maximum(np.abs(a), np.abs(b)))


# ------------------------------------------------------------------------------------------------ the reference side (no GPU)
def mode_gaps(ref):
    """gap [n, 8, 64] of an `oracle_explain` answer at n_modes = 8, as tests/golden/make_golden_modes.py writes it: (entry m - entry m + 1) /
    entry m, 1 where there is no next entry. The eighth entry's successor is not kept: its gap is 1 where the list ends there (n_positive
    says so) and 0 - not pinned by key - where a ninth leaf exists."""
    v, npos = ref["values"], ref["n_positive"]
    gap = np.ones(v.shape)
    nxt = np.arange(1, MAX_MODES)[None, :, None] < npos[:, None, :]  # entry m + 1 exists
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.maximum(0.0, (v[:, :-1] - v[:, 1:]) / v[:, :-1])
    gap[:, :-1] = np.where(nxt, g, 1.0)
    gap[:, -1] = np.where(npos > MAX_MODES, 0.0, 1.0)
    return gap


def key_exact(gap):
    """modes_ref.key_exact for every entry at once: its own gap and its predecessor's exceed TIE."""
    e = gap > TIE
    e[:, 1:] &= gap[:, :-1] > TIE
    return e


class Case:
    """One library of the sweep with the oracle's answers: `free` without a constraint, `bound` under `cons[i]` for ligand i (both at 8 modes)."""

    def __init__(self, name, model, lib, seed, constrained=True, weights=None):
        from oracle import oracle
        from pharmaconet_amd.constants import weights_vector

        self.name, self.model, self.lib, self.weights = name, model, lib, weights
        self.w7 = weights_vector(weights)
        self.C = np.array([lib.header(i)[1] for i in range(len(lib))])
        self.free = oracle.oracle_explain(model.flat, lib, self.w7, n_modes=MAX_MODES, num_threads=THREADS)
        self.free["gap"] = mode_gaps(self.free)
        rng = np.random.default_rng(seed)
        K = model.flat.num_clusters
        self.cons = []
        for i in range(len(lib)):
            rec = lib.unpack(i)
            self.cons.append(random_constraint(rng, sorted({m for lc in ligand_levels(model, rec) for m in candidates(model, rec, lc)}), K))
        self.bound = None
        if constrained:
            self.bound = oracle.oracle_explain(model.flat, lib, self.w7, n_modes=MAX_MODES, constraints=self.cons, num_threads=THREADS)
            self.bound["gap"] = mode_gaps(self.bound)
        self._tables = {}

    def levels(self, i):
        lv = self.free["levels"][i]
        return lv[lv != 0xFE].astype(np.int64)

    def reaches(self, i, key, c, value):
        """Within the tie band a key is accepted by its total: `path_score` of it is the value within 2e-6."""
        if i not in self._tables:
            rec = self.lib.unpack(i)
            self._tables[i] = (rec, Tables(self.model, rec, self.w7))
        rec, T = self._tables[i]
        return abs(path_score(self.model, rec, self.w7, self.levels(i), key, c, T) - value) <= RTOL * value


def sweep_cases(conformers, weights=None, libraries=LIBRARIES):
    """The two libraries of test_every_lane_shape_matches_the_oracle at this conformer count (or their first ligands: the generator draws
    every ligand from a stream of its own) under the type weights `weights`: computed once, shared, never written to."""
    return _sweep_cases(conformers, None if weights is None else tuple(sorted(weights.items())), tuple(libraries))


@functools.lru_cache(maxsize=None)
def _sweep_cases(conformers, weight_items, libraries):
    from tools.synthetic import synthetic_library

    out = []
    for name, n in libraries:
        model, _, _, _ = load_golden(name)
        lib = synthetic_library(n, num_conformers=conformers, model_nodes=_model_nodes(model), active_fraction=0.5, seed=5000 + conformers)
        out.append(Case(name, model, lib, 5000 + conformers, weights=None if weight_items is None else dict(weight_items)))
    return tuple(out)


def honest(cases):
    """The condition that keeps the sweep honest, from the oracle's output alone: more than half of the library scores, and at least half of
    the positive entries are compared by key, not by total. Returns the shares (maxima, modes) over the parameter's libraries."""
    for case in cases:
        assert np.count_nonzero(case.free["scores"]) > len(case.lib) // 2, case.name
    pos = np.concatenate([c.free["values"][c.free["values"] > 0] for c in cases])
    assert pos.size > 0
    top = np.concatenate([(c.free["gap"][:, 0] > TIE)[c.free["values"][:, 0] > 0] for c in cases])
    exact = np.concatenate([key_exact(c.free["gap"])[c.free["values"] > 0] for c in cases])
    assert top.mean() >= 0.5 and exact.mean() >= 0.5, (top.mean(), exact.mean())
    return float(top.mean()), float(exact.mean())


# ------------------------------------------------------------------------------------------------ the comparisons
def check_levels(case, got, i):
    assert got.tolist() == case.levels(i).tolist(), (case.name, i)


def check_keys(case, i, got, ref_keys, ref_values, exact, con, what):
    """got [M, C, nl] against the oracle's keys [M, C, 20] (uint8) and values [M, C]: all -1 where the value is 0; equal where `exact`;
    elsewhere equal, or a key whose path_score is the oracle's value; under a constraint every key qualifies. Returns (exact, by total)."""
    nl = got.shape[-1]
    want = ref_keys[..., :nl].astype(np.int64)
    want[want == 0xFF] = NONE
    pos = ref_values > 0
    assert (got[~pos] == NONE).all(), (case.name, i, what)
    assert np.array_equal(got[exact & pos], want[exact & pos]), (case.name, i, what, np.argwhere((got != want).any(axis=-1) & exact & pos).tolist())
    loose = 0
    for m, c in np.argwhere(pos):
        if con is not None:
            assert qualifies(got[m, c], *con), (case.name, i, what, m, c)
        if not exact[m, c] and not np.array_equal(got[m, c], want[m, c]):
            assert case.reaches(i, got[m, c], c, ref_values[m, c]), (case.name, i, what, m, c)
            loose += 1
    return int((exact & pos).sum()), loose


def check_explanation_row(case, ex, r, i, ref, con, what, worst):
    C = int(case.C[i])
    assert ex.status[r] == 0, (case.name, i, what)
    check_levels(case, ex.levels[r], i)
    got, want = ex.conf_max[r], ref["values"][i, 0, :C]
    assert got.shape == (C,) and np.array_equal(got == 0, want == 0), (case.name, i, what)
    nz = want > 0
    if nz.any():
        worst[0] = max(worst[0], float((np.abs(got[nz] - want[nz]) / want[nz]).max()))
    assert np.allclose(got, want, rtol=RTOL, atol=0), (case.name, i, what, got, want)
    assert ex.best_conformer[r] == int(np.argmax(got)), (case.name, i, what)
    return check_keys(case, i, ex.match[r][None], ref["keys"][i, :1, :C], want[None], (ref["gap"][i, :1, :C] > TIE), con, what)


def check_modes_row(case, ms, r, i, M, ref, con, what, worst):
    C = int(case.C[i])
    assert ms.status[r] == 0, (case.name, i, what)
    check_levels(case, ms.levels[r], i)
    got, want = ms.values[r], ref["values"][i, :M, :C]
    assert got.shape == (M, C) and np.array_equal(got == 0, want == 0), (case.name, i, what)
    nz = want > 0
    if nz.any():
        worst[0] = max(worst[0], float((np.abs(got[nz] - want[nz]) / want[nz]).max()))
    assert np.allclose(got, want, rtol=RTOL, atol=0), (case.name, i, what)
    assert ms.count(r).tolist() == np.minimum(M, ref["n_positive"][i, :C]).tolist(), (case.name, i, what)
    assert ms.best_conformer[r] == int(np.argmax(got[0])), (case.name, i, what)
    exact = key_exact(ref["gap"][i : i + 1, :, :C])[0, :M]  # (M < 8: every gap it needs is among the oracle's eight; M = 8: mode_gaps' rule for the last)
    return check_keys(case, i, ms.match[r], ref["keys"][i, :M, :C], want, exact, con, what)


def same_as_explain(ms, r, ex, q):
    return (np.array_equal(ms.values[r][0], ex.conf_max[q]) and np.array_equal(ms.match[r][0], ex.match[q]) and np.array_equal(ms.levels[r], ex.levels[q])
            and ms.best_conformer[r] == ex.best_conformer[q] and ms.status[r] == ex.status[q])


def run_all_three(case, modes=(1, 4, 8), constrained_modes=4):
    """Every ligand of the case through explain, explain under its own constraint, and explain_modes (each M, and `constrained_modes` under
    the constraint). Returns the worst relative errors (maxima, constrained maxima, mode values) and the key counts (exact, by total)."""
    from pharmaconet_amd.engine import DeviceLibrary, explain, explain_modes, screen

    n = len(case.lib)
    idx = np.arange(n)
    dlib = DeviceLibrary(case.lib)
    w_max, w_con, w_modes = [0.0], [0.0], [0.0]
    keys = np.zeros(2, np.int64)
    ex = explain(case.model, dlib, idx, weights=case.weights)
    sc = screen(case.model, dlib, weights=case.weights, float64=True).scores.cpu().numpy()
    for i in idx:
        keys += check_explanation_row(case, ex, i, i, case.free, None, "explain", w_max)
        assert ulp_close(ex.conf_max[i].mean(), sc[i]), (case.name, i, ex.conf_max[i].mean(), sc[i])
    for M in modes:
        ms = explain_modes(case.model, dlib, idx, modes=M, weights=case.weights)
        for i in idx:
            keys += check_modes_row(case, ms, i, i, M, case.free, None, f"modes={M}", w_modes)
            assert same_as_explain(ms, i, ex, i), (case.name, i, M)
    changed = 0
    for i in idx:
        require, exclude = case.cons[i]
        cx = explain(case.model, dlib, [i], weights=case.weights, require=require, exclude=exclude)
        keys += check_explanation_row(case, cx, 0, i, case.bound, case.cons[i], "constrained", w_con)
        assert (cx.conf_max[0] <= ex.conf_max[i]).all(), (case.name, i, require, exclude)
        changed += not np.array_equal(cx.conf_max[0], ex.conf_max[i])
        ms = explain_modes(case.model, dlib, [i], modes=constrained_modes, weights=case.weights, require=require, exclude=exclude)
        keys += check_modes_row(case, ms, 0, i, constrained_modes, case.bound, case.cons[i], f"constrained modes={constrained_modes}", w_modes)
        assert same_as_explain(ms, 0, cx, 0), (case.name, i, "constrained")
    assert changed > 0, case.name  # the constraints bite
    return w_max[0], w_con[0], w_modes[0], keys


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("conformers", CONFORMERS)
def test_explain_family_matches_the_oracle_at_every_lane_shape(conformers):
    """C = 2 ... 48 (G = 2 ... 64, groups full and partly filled), both models, every ligand: status, levels, maxima (2e-6, 0 exactly where the
    oracle's are 0), the best conformer, the mean against pmx_score_f64 (4 ulp), keys by the gap rule, all of it again under one seeded
    constraint per ligand (and never above the unconstrained maximum), and the ranked lists of explain_modes at M = 1, 4, 8 (and 4 under the
    constraint) with mode 0 bit for bit explain's answer."""
    cases = sweep_cases(conformers)
    top, exact = honest(cases)
    for case in cases:
        w_max, w_con, w_modes, keys = run_all_three(case)
        print(f"C={conformers} {case.name}: worst relative error maxima {w_max:.2e}, constrained maxima {w_con:.2e}, mode values {w_modes:.2e}; "
              f"{keys[0]} keys compared exactly, {keys[1]} by total; key-exact share of the oracle's entries: maxima {top:.3f}, modes {exact:.3f}")
        assert keys[0] > 0


@pytest.mark.parametrize("wname", SPREAD_WEIGHTS)
@pytest.mark.parametrize("conformers", SPREAD_CONFORMERS)
def test_explain_family_under_spread_weights(conformers, wname):
    """explain_kernel<G, true, *>: type weights a factor 1000 apart, so pair items take the term-by-term tails (`pair_tails`, csrc/pmx_api.hip).
    Everything the test above checks, on the first 64 and 24 ligands of its libraries, at one mode count - and the mean against
    pmx_score_f64 now holds across the two deciders of the arm (explain_screen and score_screen)."""
    cases = sweep_cases(conformers, WEIGHT_SETS[wname], SPREAD_LIBRARIES)
    top, exact = honest(cases)
    for case in cases:
        w_max, w_con, w_modes, keys = run_all_three(case, modes=(8,), constrained_modes=4)
        print(f"C={conformers} [{wname}] {case.name}: worst relative error maxima {w_max:.2e}, constrained maxima {w_con:.2e}, mode values {w_modes:.2e}; "
              f"{keys[0]} keys compared exactly, {keys[1]} by total; key-exact share of the oracle's entries: maxima {top:.3f}, modes {exact:.3f}")
        assert keys[0] > 0


@pytest.mark.parametrize("conformers", SHAPES)
def test_explain_takes_the_tail_arm(conformers, monkeypatch):
    """The test that fails if the explain kernels ignore `tails`: the libraries of test_gpu_tail_shapes.py (one heavy item swept through its
    tails, on the grid where the tabulated tail alone is off by 1e-5) through explain and explain_modes(modes=2), on the two-cluster model
    as `engine.screen` takes it there (an object with `.flat`). Maxima and mode values at 2e-6 with the oracle's zeros, mode 0 bit for bit
    explain; with PMX_PAIR_TAILS=0 other bits in a maximum of a record that is mostly that one tail item; and in both settings the mean
    within 4 ulp of pmx_score_f64, which decides the arm on its own."""
    from pharmaconet_amd.engine import DeviceLibrary, explain, explain_modes, screen

    wname, sigma_min_to = PAIR_SHAPE_SETS[0]
    wdict = WEIGHT_SETS[wname]
    cases, refs = pair_shape_cases(wname, sigma_min_to, conformers), pair_shape_explained(wname, sigma_min_to, conformers)
    assert len(cases) == 6 and sum(int(c.mostly_tail.sum()) for c in cases) > 0
    worst, worst_off, n_differ = 0.0, 0.0, 0
    for c, ref in zip(cases, refs):
        shim = _Shim(c.flat)
        dlib = DeviceLibrary(c.lib)
        idx = np.arange(len(c.lib))
        want = ref["values"][:, :, :conformers]  # [n, 2, C]
        assert (want[:, 0] > 0).all(), (c.a, c.b)

        def family():
            ex = explain(shim, dlib, idx, weights=wdict)
            ms = explain_modes(shim, dlib, idx, modes=2, weights=wdict)
            sc = screen(shim, dlib, weights=wdict, float64=True).scores.cpu().numpy()
            assert (ex.status == 0).all() and (ms.status == 0).all(), (c.a, c.b)
            for i in idx:
                assert same_as_explain(ms, i, ex, i), (c.a, c.b, i)
            conf_max, values = np.stack(ex.conf_max), np.stack(ms.values)
            assert ulp_close(conf_max.mean(axis=1), sc).all(), (c.a, c.b)
            return conf_max, values

        conf_max, values = family()
        assert conf_max.shape == want[:, 0].shape and values.shape == want.shape
        assert np.array_equal(values == 0, want == 0), (c.a, c.b)
        nz = want > 0
        worst = max(worst, float((np.abs(values[nz] - want[nz]) / want[nz]).max()))
        assert np.allclose(conf_max, want[:, 0], rtol=RTOL, atol=0) and np.allclose(values, want, rtol=RTOL, atol=0), (c.a, c.b, worst)
        monkeypatch.setenv("PMX_PAIR_TAILS", "0")
        off, _ = family()
        monkeypatch.delenv("PMX_PAIR_TAILS")
        worst_off = max(worst_off, float((np.abs(off - want[:, 0]) / want[:, 0]).max()))
        n_differ += int((conf_max != off).any(axis=1)[c.mostly_tail].sum())
        dlib.close()
    print(f"C={conformers} [{wname}, sigma_min {sigma_min_to}]: worst relative error of the mode values {worst:.2e} (maxima with the tabulated tails "
          f"alone, PMX_PAIR_TAILS=0: {worst_off:.2e}); {n_differ} mostly-tail records change with the arm")
    assert n_differ > 0, "no mostly-tail maximum depends on the arm"


def raw_call(model, dlib, idx, modes=0, constraint=None):
    """pmx_explain / pmx_explain_constrained / pmx_explain_modes through _ffi on buffers filled with a pattern no answer holds: the raw
    (values [n, max(modes, 1), 64], keys [n, max(modes, 1), 64, 20], levels [n, 20], best [n], status [n])."""
    import torch

    from pharmaconet_amd import _ffi
    from pharmaconet_amd.engine import _constraint_struct, _weights_array, device_model, normalize_constraint

    lib = _ffi.load()
    tdev = torch.device("cuda", dlib.device)
    mh = device_model(model, dlib.device)
    n, M = len(idx), max(modes, 1)
    lig = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).to(tdev)
    values = torch.full((n, M, 64), 7.25, dtype=torch.float64, device=tdev)
    keys = torch.full((n, M, 64, 20), 0x55, dtype=torch.uint8, device=tdev)
    levels = torch.full((n, 20), 0x55, dtype=torch.uint8, device=tdev)
    best = torch.full((n,), -7, dtype=torch.int32, device=tdev)
    status = torch.full((n,), -7, dtype=torch.int32, device=tdev)
    con = ctypes.byref(_constraint_struct(*normalize_constraint(*constraint))) if constraint is not None else None
    with torch.cuda.device(tdev):
        stream = torch.cuda.current_stream(tdev)
        outs = (lig.data_ptr(), n, values.data_ptr(), keys.data_ptr(), levels.data_ptr(), best.data_ptr(), status.data_ptr(), ctypes.c_void_p(stream.cuda_stream))
        if modes:
            _ffi.check(lib.pmx_explain_modes(mh.handle, dlib.handle, _weights_array(None), con, modes, *outs))
        elif constraint is not None:
            _ffi.check(lib.pmx_explain_constrained(mh.handle, dlib.handle, _weights_array(None), con, *outs))
        else:
            _ffi.check(lib.pmx_explain(mh.handle, dlib.handle, _weights_array(None), *outs))
        stream.synchronize()
    return tuple(t.cpu().numpy() for t in (values, keys, levels, best, status))


@functools.lru_cache(maxsize=None)
def mixed_case():
    """One library of 20-ligand parts with 1, 3, 20 and 33 conformers: G = 64 with ligands that fill 1, 3, 20 and 33 lanes."""
    from pharmaconet_amd import PackedLibrary
    from tools.synthetic import synthetic_library

    model, _, _, _ = load_golden("set_6oim_c8")
    records = []
    for C in (1, 3, 20, 33):
        part = synthetic_library(20, num_conformers=C, model_nodes=_model_nodes(model), active_fraction=0.5, seed=6000 + C)
        records += [part.record(i) for i in range(len(part))]
    return Case("mixed", model, PackedLibrary.from_records(records), 6000)


def test_mixed_conformer_counts_in_one_library():
    """Ligands of 1, 3, 20 and 33 conformers walked by the 64-lane kernels: all three calls against the oracle, and on the raw output
    buffers lanes c >= C of every row hold 0.0 and 0xFF (include/pmx.h), levels past nl 0xFE, keys past nl 0xFF."""
    from pharmaconet_amd.engine import DeviceLibrary

    case = mixed_case()
    assert sorted(set(case.C.tolist())) == [1, 3, 20, 33] and np.count_nonzero(case.free["scores"]) > len(case.lib) // 2
    for C in (1, 3, 20, 33):
        assert np.count_nonzero(case.free["scores"][case.C == C]) > 0  # every part has ligands that score
    w_max, w_con, w_modes, keys = run_all_three(case)
    print(f"mixed C=1/3/20/33: worst relative error maxima {w_max:.2e}, constrained maxima {w_con:.2e}, mode values {w_modes:.2e}; "
          f"{keys[0]} keys compared exactly, {keys[1]} by total")
    assert keys[0] > 0
    dlib = DeviceLibrary(case.lib)
    idx = np.arange(len(case.lib))
    most = np.bincount(case.free["keys"][:, 0][case.free["keys"][:, 0] < 0xFE].astype(np.int64)).argsort()[::-1]
    con = ([[int(most[0]), int(most[1])]], [int(most[2])])
    beyond = np.arange(64)[None, :] >= case.C[:, None]  # [n, 64]: lanes that are no conformer of the row's ligand
    nl = np.count_nonzero(case.free["levels"] != 0xFE, axis=1)
    for modes, constraint in ((0, None), (0, con), (1, None), (5, None), (8, con)):
        values, keys_raw, levels, best, status = raw_call(case.model, dlib, idx, modes, constraint)
        what = (modes, constraint)
        assert (status == 0).all() and ((best >= 0) & (best < case.C)).all(), what
        assert np.array_equal(levels, case.free["levels"]), what
        for m in range(max(modes, 1)):
            assert (values[:, m][beyond] == 0.0).all() and (keys_raw[:, m][beyond] == 0xFF).all(), what
            assert np.isfinite(values[:, m]).all() and (values[:, m] >= 0).all(), what
            zero = values[:, m] == 0
            assert (keys_raw[:, m][zero] == 0xFF).all(), what
            for i in idx:
                assert (keys_raw[i, m, :, nl[i]:] == 0xFF).all(), what
        if constraint is None:  # the live lanes are the oracle's
            want = case.free["values"][:, : max(modes, 1)]
            assert np.allclose(values, want, rtol=RTOL, atol=0) and np.array_equal(values == 0, want == 0), what


@pytest.mark.parametrize("conformers,wname", [(3, "default"), (16, "default"), (33, "default"), (3, "charged_heavy"), (16, "charged_heavy"), (33, "charged_heavy")],
                         ids=["3", "16", "33", "3-charged_heavy", "16-charged_heavy", "33-charged_heavy"])
def test_attribution_of_explained_ligands_at_other_shapes(conformers, wname):
    """`Explanation.attribution` of every explained ligand at G = 4, 16 and 64: pmx_attribute's total of the reported key at the best
    conformer is that conformer's maximum (2e-6, test_gpu_attribution.py::test_attribution_of_explained_ligands), its shares add up to it.
    Under `charged_heavy` this is the cross-check of the TAILS design on realistic ligands: pmx_attribute evaluates every item term by
    term, explain reads the tables and takes the term-by-term tails."""
    from pharmaconet_amd.engine import DeviceLibrary, explain

    attributed = 0
    weights = WEIGHT_SETS[wname]
    for case in sweep_cases(conformers) if weights is None else sweep_cases(conformers, weights, SPREAD_LIBRARIES):
        dlib = DeviceLibrary(case.lib)
        ex = explain(case.model, dlib, np.arange(len(case.lib)), weights=weights)
        assert (ex.status == 0).all()
        at = ex.attribution(case.model, dlib, weights=weights)
        assert len(at) == len(ex) and (at.status == 0).all(), case.name
        worst = 0.0
        for r, i in enumerate(at.rows):
            assert at.indices[r] == ex.indices[i] and at.conformers[r] == ex.best_conformer[i]
            assert at.levels[r].tolist() == ex.levels[i].tolist()
            cm, tot = float(ex.conf_max[i][ex.best_conformer[i]]), float(at.total[r])
            assert abs(tot - cm) <= RTOL * cm, (case.name, i, tot, cm)
            if cm > 0:
                worst = max(worst, abs(tot - cm) / cm)
                attributed += 1
            n, nl = len(at.node[r]), len(at.levels[r])
            P, E = n * (n - 1) // 2, nl * (nl + 1) // 2
            assert (at.node[r] >= 0).all() and abs(float(at.node[r].sum()) - tot) <= (5 * P + 2 * E + n) * np.spacing(tot), (case.name, i)
        print(f"C={conformers} {case.name}: attribution total against the explained maximum, worst relative error {worst:.2e}")
    assert attributed > 0
