"""That the cases of tests/model_cases.py reach what tests/test_gpu_hand_models.py runs them for, from the oracle and the host tables alone:
conditions on the inputs, checked without a GPU.

Measured here (share of the rows with a non-zero score on which the oracle's scores of the model and of its transpose differ by more than
1e-3 of the larger): A1 0.64 (C = 1, 3, 8, 33) and 0.76 (C = 64); A2 on cluster {0, 2} 1.0 at every C, on cluster {0, 1} none (the largest
difference there is 6e-8); A3 with the factors 0.05 and 0.2 0.97 (set_6oim_c8), 1.0 (set_6oim_c64), 1.0 (set_l110_c8). All 9 complex
cells of model_6oim_like are reached; in 3 of them (subsets 14 x 7 cell 25, 26 x 15 and 26 x 17 cell 28) the majority count decides a score, in
the other 6 the other assignment of the two ligand clusters to the two model clusters scores wherever the aimed one fails."""

import numpy as np
import pytest

import model_cases as mc
from test_model_tables_cpu import subset_nodes, up

SHOWS = 1e-3  # 500 times the parity tolerance


@pytest.fixture(scope="module", autouse=True)
def built(oracle):
    mc.host_lib()


def transpose_difference(case):
    """(rows where either score is non-zero, the difference there relative to the larger score)."""
    other = mc.oracle_scores(mc.transposed(case.flat), case.lib)
    rows = (case.ref != 0) | (other != 0)
    return rows, np.abs(case.ref - other)[rows] / np.maximum(np.abs(case.ref), np.abs(other))[rows]


# ------------------------------------------------------------------------------------------------ A
def test_asymmetric_models_are_square_in_the_tables():
    for case in (mc.a1_cases()[0],) + mc.a2_cases()[:: len(mc.CONFORMERS)] + mc.a3_cases()[1:]:
        t = mc.host_tables(case.flat)
        assert t["symmetric"] == 0 and t["NF"] == t["NS"] * t["NS"], case.name


def test_a1_the_transpose_shows():
    for case in mc.a1_cases():
        pairs, which = case.aim
        assert set(pairs) == {(m0, m1) for m0 in (1, 16, 17) for m1 in (1, 16, 17)}  # both cluster orders of every pair
        assert case.dist.shape == (len(case.lib), int(case.name.split("_c")[1])) and case.dist.max() >= mc.table_range(case.flat)
        rows, rd = transpose_difference(case)
        print(case.name, len(case.lib), "records,", int(rows.sum()), "non-zero, share", float((rd > SHOWS).mean()))
        assert rows.sum() >= 16 and (rd > SHOWS).mean() >= 0.5, case.name


def test_a2_the_transpose_shows_between_two_types_and_not_within_one():
    for case in mc.a2_cases():
        a, same_type = case.aim
        rows, rd = transpose_difference(case)
        assert rows.any()
        if same_type:  # both subsets are {0, 1} and the sum runs over both directions
            assert rd.max() <= 1e-6, case.name
        else:
            assert (rd > SHOWS).mean() >= 0.5, case.name


def test_a3_the_transpose_shows():
    assert (mc.A3_MEAN_FACTOR, mc.A3_STD_FACTOR) == (0.05, 0.2)
    for case in mc.a3_cases():
        full = mc.golden_flat(case.name.startswith("a3_set_l110") and "model_large110" or "model_6oim_like")
        low = np.tril(np.ones((full.num_nodes,) * 2, dtype=bool))
        assert np.array_equal(case.flat.edge_mean[low], full.edge_mean[low]) and np.array_equal(case.flat.edge_std[low], full.edge_std[low])
        assert (case.flat.edge_std > 0).all() and case.flat.edge_mean.dtype == case.flat.edge_std.dtype == np.float32
        rows, rd = transpose_difference(case)
        print(case.name, int(rows.sum()), "non-zero, share", float((rd > SHOWS).mean()))
        assert rows.any() and (rd > SHOWS).mean() >= 0.5, case.name
    assert mc.a3_cases()[2].flat.num_nodes > 64  # node sets of two words


# ------------------------------------------------------------------------------------------------ B
def test_b1_pass_gap_pass_inside_the_cell():
    c1, c64 = mc.b1_cases()
    d = c1.dist[:, 0]
    assert np.all(np.diff(d) > 0) and np.array_equal(c64.dist.reshape(-1)[: len(d)], d)
    x0, last = c1.aim
    inside = (d >= x0) & (d <= last)
    assert d[np.flatnonzero(inside)[0] - 1] == mc.down(x0) and d[np.flatnonzero(inside)[-1] + 1] == up(last)
    for e in mc.gap_edges(c1.flat):
        assert np.isin(mc.around(e, 32), d).all()
    assert inside.sum() >= 2048
    alive, din = c1.ref[inside] > 0, d[inside]
    turns = np.flatnonzero(alive[1:] != alive[:-1])
    assert len(turns) == 2 and alive[0] and not alive[turns[0] + 1] and alive[-1]  # non-zero, zero, non-zero
    for k in turns:  # both transitions between two floats that are neighbours
        assert din[k + 1] == up(din[k])
    lo1, hi1, lo2, hi2 = mc.gap_edges(c1.flat)
    assert din[turns[0]] == np.float32(hi1) and din[turns[1] + 1] == np.float32(lo2)
    assert c64.ref.max() > 0 and len(c64.lib) == -(-len(d) // 64)


def test_b1_and_b3_land_in_cells_of_two_windows():
    c1, _ = mc.b1_cases()
    t, win = mc.aimed_windows(c1.flat, 1, 1)
    assert t["n_complex_cells"] >= 1
    assert subset_nodes(t, int(t["sidtab"][1])).tolist() == [0] and subset_nodes(t, int(t["sidtab"][128 + 1])).tolist() == [1, 2]
    d = c1.dist[:, 0]
    inside = (d >= c1.aim[0]) & (d <= c1.aim[1])
    assert (mc.cell_of(t, d[inside]) == mc.B1_CELL).all() and np.isnan(win[mc.B1_CELL]).all()
    cells = mc.b3_cases()
    full = mc.host_tables(mc.golden_flat("model_6oim_like"))
    assert len(cells) == full["n_complex_cells"] == 9
    n_decided = 0
    for c1, c64 in cells:
        sa, sb, i, ca, cb, m0, m1, decided = c1.aim
        t, win = mc.aimed_windows(c1.flat, m0, m1)
        assert t["n_complex_cells"] >= 1 and np.isnan(win[i]).all()
        # the masks select the cell's two subsets, in clusters 0 and 1 of the reduced model
        assert subset_nodes(t, int(t["sidtab"][m0])).tolist() == subset_nodes(full, sa).tolist()
        assert subset_nodes(t, int(t["sidtab"][128 + m1])).tolist() == subset_nodes(full, sb).tolist()
        for c in (c1, c64):
            assert (mc.cell_of(t, c.dist) == i).all(), c.name
        assert len(np.unique(c1.dist)) >= 256 and np.array_equal(np.unique(c64.dist), np.unique(c1.dist))
        assert decided == bool((c1.ref == 0).any() and (c1.ref > 0).any())
        n_decided += decided
        print(c1.name, "decided" if decided else "reached", int((c1.ref > 0).sum()), "non-zero,", int((c1.ref == 0).sum()), "zero")
    assert n_decided >= 3  # (reached: 9 of 9; the issue asks for 6)


def test_b2_has_no_cell_of_two_windows():
    c1, c64 = mc.b2_cases()
    t = mc.host_tables(c1.flat)
    assert t["n_complex_cells"] == 0 and not np.isnan(t["win"]).any()
    d = c1.dist[:, 0]
    lo1, hi1, lo2, hi2 = mc.gap_edges(c1.flat)
    assert up(hi1) == np.float32(4.0)  # the first window ends with the last float of its cell
    for e in (lo1, hi1, lo2, hi2, 4.0):
        assert np.isin(mc.around(e, 32), d).all()
    alive = dict(zip(d.tolist(), (c1.ref > 0).tolist()))
    assert alive[float(np.float32(hi1))] and not alive[4.0] and not alive[float(mc.down(lo2))] and alive[float(np.float32(lo2))]


# ------------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("model", mc.C_MODELS)
def test_c_a_float_decides(model):
    single, multi = mc.c_functions(model)
    assert len(single) == mc.C_SINGLE and len(multi) == mc.C_MULTI
    t = mc.host_tables(mc.golden_flat(model))
    nm = t["Nm"]
    n_ends = 0
    for k, fn in enumerate(single + multi):
        edges = [m * nm + n for m in fn.A for n in fn.B]
        assert fn.a != fn.b and len(edges) == len(fn.windows) and (len(edges) == 1) == (k < mc.C_SINGLE)
        assert [w[0] for w in fn.windows] == t["wlo"][edges].tolist() and [w[1] for w in fn.windows] == t["whi"][edges].tolist()
        assert len(fn.case.lib) == len(edges) * 2 * (2 * mc.C_ULPS + 1) and fn.case.dist.shape[1] == 1
        decided, constant = mc.window_ends(fn)
        if len(edges) == 1:
            assert decided.all()
        else:
            assert decided.sum() >= 2 and (decided | constant).all()
        n_ends += int(decided.sum())
    print(model, n_ends, "window ends decided by a float;", sorted(len(fn.windows) for fn in multi), "node pairs in the functions of several")


# ------------------------------------------------------------------------------------------------ D
def test_d_the_limits_are_reached():
    case = mc.d_case()
    flat = case.flat
    t = mc.host_tables(flat)
    assert (t["Nm"], t["K"]) == (mc.D_NODES, mc.D_CLUSTERS) == (256, 128)
    lists = mc.cluster_lists(flat)
    assert lists[-1] == [29, 255] and all(lists) and {n for nodes in lists for n in nodes} >= {0, 255}
    assert max(n // 64 for n in lists[1]) > min(n // 64 for n in lists[1])  # a cluster's members lie in different node words
    assert len(case.lib) == 16
    reached = set()
    for r in range(16):
        rec = case.lib.unpack(r)
        assert int(rec["n_clusters"]) == 2
        for mask in {int(x) for x in rec["typemask"]}:
            cand = int(t["tclus"][2 * mask]) | int(t["tclus"][2 * mask + 1]) << 64
            reached |= {a for a in mc.D_REACH if cand >> a & 1}
    assert reached == set(mc.D_REACH)
    print("oracle", case.ref.tolist())
    assert (case.ref > 0).sum() >= 8
