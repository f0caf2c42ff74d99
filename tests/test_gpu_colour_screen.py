"""The colour calls where a screen's user meets them, on a golden set: `ScreeningResult.combo_overlay`, `fitting(colour=...)`,
`PharmacophoreModel.scoring_colour`, and the two side CSVs of the command line (`--pose_colour`, `--combo_out`) - each against the engine
call it is made of, bit for bit, with a check that the main CSV and the side CSVs that existed before keep their bytes next to the new flags."""

import numpy as np
import pytest

from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu


def known_binder(model, lib, tmp_path):
    """The best hit of the set, posed where the model puts it, as the known ligand: its nodes as a PDB of carbons and as a features CSV."""
    from pharmaconet_amd.engine import explain
    from pharmaconet_amd.shape import ColourFeatures

    res = model.screen(lib)
    best = int(res._best(1)[0])
    al = explain(model, lib, [best]).poses(model, lib)
    col = ColourFeatures.from_library(lib, best, int(al.conformers[0]), al.rotation[0], al.translation[0])
    csv = tmp_path / "binder.csv"
    col.to_csv(csv)
    pdb = tmp_path / "binder.pdb"
    pdb.write_text("".join(f"HETATM{i + 1:5d}  C{i % 100:<2d} LIG A   1    {x:8.3f}{y:8.3f}{z:8.3f}  1.00  0.00           C\n" for i, (x, y, z) in enumerate(col.xyz)) + "END\n")
    return res, csv, pdb


def test_screening_result_fitting_and_one_ligand(tmp_path):
    from pharmaconet_amd.engine import colour_of, combo_overlay, explain
    from pharmaconet_amd.shape import ColourFeatures, ReferenceLigand

    model, lib, _, _ = load_golden("set_6oim_c8")
    lib = lib.select(np.arange(16))
    res, csv, pdb = known_binder(model, lib, tmp_path)
    ref = ReferenceLigand.from_pdb(pdb)
    ref.colour = ColourFeatures.from_csv(csv)
    hits = res._best(6).astype(np.int64)
    al = explain(model, lib, hits).poses(model, lib)
    best = res.combo_overlay(6, ref, node_radius=1.7)
    want = combo_overlay(ref, lib, al.indices, al.conformers, starts=4, node_radius=1.7)
    assert np.array_equal(best.indices, hits) and np.array_equal(best.combo, want.combo) and np.array_equal(best.rotation, want.rotation) and np.array_equal(best.start, want.start)
    assert best.combo[0] > 1.5 and ((best.combo >= 0) & (best.combo <= 2 + 1e-12)).all() and best.colour_weight == want.colour_weight > 0
    every = res.combo_overlay(2, ref, conformers="all", node_radius=1.7, max_iter=8)
    heads = lib.headers()
    for h, hit in enumerate(hits[:2]):
        C = int(heads[hit, 1])
        each = combo_overlay(ref, lib, [hit] * C, range(C), starts=4, node_radius=1.7, max_iter=8)
        k = int(np.argmax(each.combo))
        assert every.conformers[h] == k and every.combo[h] == each.combo[k] and every.start[h] == each.start[k]
    for kw in (dict(conformers="all", starts=0), dict(conformers="some"), dict(starts=2)):
        with pytest.raises(ValueError):
            res.combo_overlay(6, ref, **kw)
    # fitting: the colour report of every posed hit, and nothing else changes
    from pharmaconet_amd.pocket import PocketAtoms

    pocket = PocketAtoms.from_pdb(GOLDEN / "pocket_6oim.pdb", centers=model.node_centers)
    with_colour = res.fitting(4, pool=12, max_clashing=2, pocket=pocket, colour=ref, colour_cover=1.5)
    assert len(with_colour.colour) == len(with_colour.poses) == 12
    assert np.array_equal(with_colour.colour.overlap, colour_of(with_colour.poses, ref, lib, cover=1.5).overlap, equal_nan=True)
    with pytest.raises(ValueError):
        res.fitting(4, pool=12, pocket=pocket, colour_cover=1.5)
    # one ligand
    one = model.scoring_colour(lib.select([int(hits[0])]), ref)
    rep = colour_of(al, ref, lib)
    assert one["overlap"] == rep.overlap[0] and one["tanimoto"] == rep.tanimoto[0] > 0.99999 and one["by_type"] == rep.by_type(0) and one["n_matched"] == rep.n_matched[0] and one["status"] == 0


def test_cli_pose_colour_and_combo_csv(tmp_path):
    from pharmaconet_amd.constants import TYPE_NAMES
    from pharmaconet_amd.engine import colour_of, combo_overlay, explain
    from pharmaconet_amd.screening import COMBO_HEADER, OVERLAY_HEADER, POSE_COLOUR_HEADER, main
    from pharmaconet_amd.shape import ColourFeatures, ReferenceLigand

    model, lib, _, _ = load_golden("set_6oim_c8")
    lib = lib.select(np.arange(16))
    libfile = tmp_path / "lib.pmxlib"
    lib.save(libfile)
    _, csv, pdb = known_binder(model, lib, tmp_path)
    args = ["-p", str(GOLDEN / "model_6oim_like.pm"), "-d", str(libfile), "--explain", "5", "--shape_level", "nodes"]
    main(args + ["-o", str(tmp_path / "plain.csv"), "--explain_out", str(tmp_path / "plain_hits.csv"), "--overlay_out", str(tmp_path / "plain_overlay.csv"), "--shape_ref", str(pdb)])
    main(args + ["-o", str(tmp_path / "with.csv"), "--explain_out", str(tmp_path / "hits.csv"), "--overlay_out", str(tmp_path / "overlay.csv"), "--shape_ref", str(pdb),
                 "--pose_colour", str(tmp_path / "colour.csv"), "--colour_ref", str(csv), "--colour_cover", "1.5", "--combo_out", str(tmp_path / "combo4.csv")])
    for a, b in (("plain.csv", "with.csv"), ("plain_hits.csv", "hits.csv"), ("plain_overlay.csv", "overlay.csv")):
        assert (tmp_path / a).read_bytes() == (tmp_path / b).read_bytes()
    base = ["-p", str(GOLDEN / "model_6oim_like.pm"), "-d", str(libfile), "-o", str(tmp_path / "y.csv")]
    for bad in (["--pose_colour", str(tmp_path / "o.csv"), "--colour_ref", str(csv)],  # no --explain
                ["--explain", "5", "--pose_colour", str(tmp_path / "o.csv")],  # no reference
                ["--explain", "5", "--colour_ref", str(csv)],  # a reference for nothing
                ["--explain", "5", "--pose_colour", str(tmp_path / "o.csv"), "--colour_ref", str(csv), "--colour_cover", "-1"],
                ["--explain", "5", "--combo_out", str(tmp_path / "o.csv"), "--colour_ref", str(csv), "--shape_level", "nodes"],  # no shape reference
                ["--explain", "5", "--combo_out", str(tmp_path / "o.csv"), "--colour_ref", str(csv), "--shape_ref", str(pdb)],  # atoms of a packed library
                ["--explain", "5", "--combo_out", str(tmp_path / "o.csv"), "--colour_ref", str(csv), "--shape_ref", str(pdb), "--shape_level", "nodes", "--combo_weight", "-1"],
                ["--explain", "5", "--combo_out", str(tmp_path / "o.csv"), "--colour_ref", str(csv), "--shape_ref", str(pdb), "--shape_level", "nodes", "--combo_weight", "heavy"]):
        with pytest.raises(SystemExit):
            main(base + bad)
    hits = [row.split(",") for row in (tmp_path / "hits.csv").read_text().splitlines()[1:]]
    names = {f"{libfile}#{i}": i for i in range(len(lib))}
    al = explain(model, lib, [names[h[1]] for h in hits]).poses(model, lib)
    col, ref = ColourFeatures.from_csv(csv), ReferenceLigand.from_pdb(pdb)
    rep = colour_of(al, col, lib, cover=1.5)
    rows = (tmp_path / "colour.csv").read_text().splitlines()
    assert rows[0] == POSE_COLOUR_HEADER == ("rank,path,conformer,stage,nodes,matched,reference_features,reference_matched,colour_overlap,colour_tanimoto,reference_fraction,"
                                             "fit_fraction," + ",".join(TYPE_NAMES)) and len(rows) == len(hits) + 1 == 6
    for r, row in enumerate(rows[1:]):
        f = row.split(",")
        assert len(f) == 19 and int(f[0]) == r + 1 and f[1] == hits[r][1] and int(f[2]) == int(al.conformers[r]) and f[3] == "fit", r
        assert [int(v) for v in f[4:8]] == [rep.n_nodes[r], rep.n_matched[r], len(col), rep.n_reference_matched[r]], r
        assert [float(v) for v in f[8:12]] == [rep.overlap[r], rep.tanimoto[r], rep.reference_fraction[r], rep.fit_fraction[r]] and repr(float(f[9])) == f[9], r
        assert [float(v) for v in f[12:]] == rep.type_overlap[r].tolist(), r
    assert float(rows[1].split(",")[9]) > 0.99999  # the best hit is the known binder, to the float32 rounding of its posed nodes
    want = {"combo4.csv": combo_overlay(ref, lib, al.indices, al.conformers, colour=col, starts=4)}
    for name, ov in want.items():
        rows = (tmp_path / name).read_text().splitlines()
        assert rows[0] == COMBO_HEADER == OVERLAY_HEADER + ",colour_tanimoto_start,colour_tanimoto,combo" and len(rows) == 6
        for r, row in enumerate(rows[1:]):
            f = row.split(",")
            assert len(f) == 30 and int(f[0]) == r + 1 and f[1] == hits[r][1] and int(f[2]) == int(al.conformers[r]) and f[3] == "nodes", (name, r)
            assert [int(v) for v in f[4:8]] == [ov.start[r], ov.n_points[r], ov.iterations[r], ov.stop[r]], (name, r)
            assert float(f[8]) == ov.tanimoto_start[r] and float(f[9]) == ov.tanimoto[r] and float(f[10]) == ov.overlap[r] and float(f[14]) == ov.shift[r], (name, r)
            assert np.array_equal(np.array([float(v) for v in f[15:24]]).reshape(3, 3), ov.rotation[r]) and np.array_equal(np.array([float(v) for v in f[24:27]]), ov.translation[r])
            assert [float(v) for v in f[27:]] == [ov.colour_tanimoto_start[r], ov.colour_tanimoto[r], ov.combo[r]] and repr(float(f[29])) == f[29], (name, r)
