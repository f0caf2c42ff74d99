"""The row formatters of the command line's side CSVs (`screening.*_rows`): functions from result objects to text lines that call no engine,
so stand-ins do - plain namespaces with the arrays and the few methods a formatter calls. Two rows: a normal hit, and one that holds NaN, -1
and empty sets. Every row has as many fields as its header; every float field is the `repr` of its float64, or `nan`; and the motion columns
sit in every row where the header names them - in the five headers that have them, the same twelve names in the same order."""

from types import SimpleNamespace as NS

import numpy as np

from pharmaconet_amd import screening as sc
from pharmaconet_amd.constants import TYPE_NAMES

NAN = float("nan")
PATHS, ORDER = ["/data/good.sdf", "/data/odd.sdf"], [7, 3]
ROTATION = np.stack([np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), np.full((3, 3), NAN)])
TRANSLATION = np.array([[1.5, -2.25, 1.0 / 3.0], [NAN, NAN, NAN]])
MOTION = [[repr(float(v)) for v in (*R.reshape(-1), *t)] for R, t in zip(ROTATION, TRANSLATION)]
TYPES = ["Hydrophobic", "Aromatic", "Cation"]  # (the model's cluster types, by model cluster)


def f64(*v):
    return np.array(v, dtype=np.float64)


def i64(*v):
    return np.array(v, dtype=np.int64)


def posed(**more):
    """Two posed rows behind the explanation's rows 0 and 1, at conformers 2 and 0."""
    return NS(rows=i64(0, 1), conformers=i64(2, 0), indices=i64(*ORDER), rotation=ROTATION, translation=TRANSLATION, **more)


AL = posed(rmsd=f64(0.1, NAN), rmsd_nodes=f64(0.05, NAN), n_nodes=i64(4, 0))
EX = NS(best_conformer=i64(2, 0), conf_max=[f64(1.0, 2.0, 3.5), f64(0.0)], levels=[i64(0, 1, 2), i64(0)],
        match=[np.array([[0, 1, -1], [0, -1, -1], [2, -1, 1]]), np.array([[-1]])])


def clash_report():
    return NS(n_points=i64(9, 0), n_clashing=i64(1, 0), n_pairs=i64(2, 0), clearance=f64(-0.3, NAN), overlap=f64(0.125, NAN), n_contacts=i64(5, 0), worst=np.array([[3, 17], [-1, -1]]),
              atom_label=lambda r, pocket: ("A:GLY12:CA", "")[r], residues=lambda r, pocket: (["A:GLY12", "A:CYS12"], [])[r])


def overlay_report(**more):
    return NS(rotation=ROTATION, translation=TRANSLATION, start=i64(2, -1), n_points=i64(9, 0), iterations=i64(12, 0), stop=i64(1, -1), tanimoto_start=f64(0.4, NAN), tanimoto=f64(0.7, NAN),
              overlap=f64(50.0, NAN), reference_overlap=f64(80.0, 80.0), self_overlap=f64(60.0, 0.0), angle=f64(0.5, NAN), shift=f64(1.25, NAN), **more)


def side_csvs():
    """(name, header, the lines of the two stand-in rows) of every side CSV."""
    ms = NS(best_conformer=i64(1, -1), values=[np.array([[1.0, 4.0], [0.5, 2.0]]), np.zeros((2, 0))], levels=[i64(0, 1), i64()],
            match=[np.array([[[0, 1], [1, 0]], [[0, -1], [-1, 2]]]), np.zeros((2, 0, 0), np.int64)], count=lambda r: (i64(2, 2), i64())[r])
    at = NS(rows=i64(0, 1), conformers=i64(2, 0), total=f64(3.5, 0.0), node=[f64(2.0, 1.5, 0.0), f64()])
    records = [dict(cluster_end=i64(1, 2, 3), typemask=i64(1, 6, 64)), dict(cluster_end=i64(), typemask=i64())]
    hs = NS(rows=i64(0, 1), total=f64(3.5, 0.0), terms=[i64(2, 0, 1), i64(0, 0, 0)], share=[f64(3.0, 0.0, 0.5), f64(0.0, 0.0, 0.0)], nodes=lambda r: (i64(0), i64())[r])
    ps = NS(conformer=i64(1, -1), mode=i64(3, -1), passes=np.array([True, False]), n_candidates=i64(12, 0), n_passing=i64(2, 0), value=f64(3.0, NAN), fraction=f64(0.75, NAN))
    refined = NS(rotation=ROTATION, translation=TRANSLATION, anchor_rmsd=f64(0.2, NAN), angle=f64(0.1, NAN), shift=f64(0.3, NAN), iterations=i64(7, 0), stop=i64(2, -1))
    fit = NS(n_nodes=i64(4, 0), n_pairs=i64(5, 0), n_in_place=i64(3, 0), n_passing=i64(4, 0), fit=f64(2.5, NAN), ideal=f64(4.0, NAN), fraction=f64(0.625, NAN), best_fit=f64(2.75, NAN),
             best_fraction=f64(0.6875, NAN), occupied=lambda r: (i64(0, 2), i64())[r])
    shape = NS(n_points=i64(9, 0), n_covered=i64(7, 0), n_reference_covered=i64(30, 0), overlap=f64(50.0, NAN), tanimoto=f64(0.7, NAN), reference_fraction=f64(0.625, NAN),
               fit_fraction=f64(0.8, 0.0), rms_to_reference=f64(1.1, NAN), rms_from_reference=f64(1.3, NAN))
    colour = NS(n_nodes=i64(4, 0), n_matched=i64(3, 0), n_reference_matched=i64(5, 0), overlap=f64(2.0, NAN), tanimoto=f64(0.5, NAN), reference_fraction=f64(0.4, NAN), fit_fraction=f64(0.6, NAN),
                type_overlap=np.stack([np.linspace(0.0, 1.0, len(TYPE_NAMES)), np.full(len(TYPE_NAMES), NAN)]))
    combo = overlay_report(colour_tanimoto_start=f64(0.2, NAN), colour_tanimoto=f64(0.5, NAN), combo=f64(1.2, NAN))
    return [
        ("explain", sc.EXPLAIN_HEADER, sc.explain_rows(PATHS, f64(11.5, 0.0), EX, TYPES)),
        ("modes", sc.MODES_HEADER, sc.modes_rows(PATHS, ms, TYPES)),
        ("explain_nodes", sc.EXPLAIN_NODES_HEADER, sc.explain_nodes_rows(PATHS, ORDER, EX, at, records)),
        ("hotspots", sc.HOTSPOTS_HEADER, sc.hotspots_rows(PATHS, hs, i64(0, 1, 6))),
        ("poses", sc.POSES_HEADER, sc.poses_rows(PATHS, AL)),
        ("pose_search", sc.POSE_SEARCH_HEADER, sc.pose_search_rows(PATHS, ps, AL, clash_report())),
        ("clashes", sc.CLASHES_HEADER, sc.clashes_rows(PATHS, AL, clash_report(), "atoms", None)),
        ("refine", sc.REFINE_HEADER, sc.refine_rows(PATHS, AL, clash_report(), refined, clash_report(), "nodes")),
        ("pose_fit", sc.POSE_FIT_HEADER, sc.pose_fit_rows(PATHS, AL, [("fit", fit), ("refined", fit)])),
        ("pose_shape", sc.POSE_SHAPE_HEADER, sc.pose_shape_rows(PATHS, AL, [("fit", shape), ("refined", shape)], "atoms", 41)),
        ("overlay", sc.OVERLAY_HEADER, sc.overlay_rows(PATHS, AL, overlay_report(), "atoms")),
        ("pose_colour", sc.POSE_COLOUR_HEADER, sc.pose_colour_rows(PATHS, AL, colour, 6)),
        ("combo", sc.COMBO_HEADER, sc.overlay_rows(PATHS, AL, combo, "nodes", combo=True)),
    ]


INTEGERS = {"rank", "index", "conformer", "best_conformer", "mode", "node", "ligand_cluster", "passes", "candidates", "passing", "clashing", "fitted_nodes", "points", "pairs", "contacts",
            "worst_point", "pairs_before", "pairs_after", "clashing_after", "iterations", "stop", "pairs", "in_place", "covered", "reference_atoms", "reference_covered", "start", "nodes",
            "matched", "reference_features", "reference_matched", "engaged"}
TEXT = {"path", "matches", "node_types", "model_cluster", "type", "level", "stage", "worst_atom", "residues", "occupied_nodes"}


def test_every_row_fits_its_header_and_every_float_is_a_repr():
    expected_lines = dict(explain=2, modes=2, explain_nodes=3, hotspots=2, poses=2, pose_search=2, clashes=2, refine=2, pose_fit=4, pose_shape=4, overlay=2, pose_colour=2, combo=2)
    for name, header, lines in side_csvs():
        columns, lines = header.split(","), list(lines)
        assert len(lines) == expected_lines[name], name
        for line in lines:
            fields = line.split(",")
            assert len(fields) == len(columns) and "\n" not in line, (name, line)
            for column, field in zip(columns, fields):
                if column in INTEGERS:
                    assert str(int(field)) == field, (name, column, field)
                elif column not in TEXT:
                    assert field == "nan" or repr(float(field)) == field, (name, column, field)
        assert {line.split(",")[columns.index("path")] for line in lines} == set(PATHS) or name in ("modes", "explain_nodes", "hotspots"), name  # (those three: nothing for the empty hit)


def test_the_odd_row_is_written_out_not_left_out():
    rows = {name: list(lines) for name, _, lines in side_csvs()}
    assert rows["explain"] == ["1,/data/good.sdf,11.5,2,3.5,0->2:Cation 2->1:Aromatic", "2,/data/odd.sdf,0.0,0,0.0,"]
    assert rows["modes"] == ["1,/data/good.sdf,0,4.0,1.0,0->1:Aromatic 1->0:Hydrophobic", "1,/data/good.sdf,1,2.0,0.5,1->2:Cation"]
    assert rows["explain_nodes"][1] == f"1,7,/data/good.sdf,2,1,{TYPE_NAMES[1]}|{TYPE_NAMES[2]},1,,1.5," + repr(1.5 / 3.5)  # (ligand cluster 1 is matched to None)
    assert rows["clashes"][1] == "2,/data/odd.sdf,0,atoms,0,0,0,nan,nan,0,-1,,"
    assert rows["pose_fit"][3].endswith(",nan,nan,nan,nan,nan,") and rows["pose_fit"][0].endswith(",0;2")
    assert rows["overlay"][1].split(",")[8:15] == ["nan", "nan", "nan", "nan", "0.0", "nan", "nan"]  # (a hit without points: nothing of it lies inside the reference)


def test_motion_columns_sit_where_the_header_names_them():
    names = sc.MOTION_COLUMNS.split(",")
    assert names == ["r00", "r01", "r02", "r10", "r11", "r12", "r20", "r21", "r22", "tx", "ty", "tz"]
    with_motion = [(name, header, list(lines)) for name, header, lines in side_csvs() if "r00" in header]
    assert [name for name, _, _ in with_motion] == ["poses", "pose_search", "refine", "overlay", "combo"]
    for name, header, lines in with_motion:
        columns = header.split(",")
        at = columns.index("r00")
        assert columns[at : at + 12] == names and columns.count("r00") == 1, name
        assert [line.split(",")[at : at + 12] for line in lines] == MOTION, name
    for a, b in (("POSE_SEARCH_HEADER", "REFINE_HEADER"), ("REFINE_HEADER", "OVERLAY_HEADER"), ("OVERLAY_HEADER", "COMBO_HEADER")):  # after fifteen columns in these four
        assert getattr(sc, a).split(",").index("r00") == getattr(sc, b).split(",").index("r00") == 15
