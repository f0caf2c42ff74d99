"""The command lines `screening.main` refuses, pinned to their messages: every one exits with status 2 before anything touches the GPU -
`torch` is never imported. One fault per command line, so the message does not depend on the order of the checks. The cases are the `bad`
lists of the command-line tests next to each report, and one line per `parser.error` that is reached before the model is read; the messages
are those of the commit before the side reports were put behind one hit context. `{t}` stands for the test's directory, `{g}` for
tests/golden. The library is `set_6oim_c5.pmxlib`, copied, with a names file `/data/mol_<i>.sdf` and no `.atoms` file beside it."""

import json
import shutil
import subprocess
import sys
from pathlib import Path

from conftest import GOLDEN

REPO = Path(__file__).resolve().parent.parent
BASE = ["-p", "{g}/model_6oim_like.pm", "-d", "{t}/lib.pmxlib", "-o", "{t}/out.csv"]
POCKET, LIGAND, COLOUR = ["--protein", "{g}/pocket_6oim.pdb"], ["--shape_ref", "{g}/ligand_6oim_mov.pdb"], ["--colour_ref", "{t}/binder.csv"]
NEEDS_EXPLAIN = " needs --explain K"
NO_ATOMS = " atoms takes the hits' atoms from {t}/lib.pmxlib.atoms, which does not exist (--save_top writes it from a library directory"

CASES = [
    # a side report of the explained hits without --explain K
    (["--explain_nodes", "{t}/n.csv"], "--explain_nodes" + NEEDS_EXPLAIN),
    (["--poses", "{t}/p.csv"], "--poses" + NEEDS_EXPLAIN),
    (["--clashes", "{t}/c.csv", *POCKET, "--clash_level", "nodes"], "--clashes" + NEEDS_EXPLAIN),
    ([*POCKET, "--refine_out", "{t}/r.csv", "--clash_level", "nodes"], "--refine_out" + NEEDS_EXPLAIN),
    (["--pose_search", "{t}/s.csv"], "--pose_search" + NEEDS_EXPLAIN),
    (["--pose_fit", "{t}/f.csv"], "--pose_fit" + NEEDS_EXPLAIN),
    (["--pose_shape", "{t}/s.csv", *LIGAND], "--pose_shape" + NEEDS_EXPLAIN),
    (["--overlay_out", "{t}/o.csv", *LIGAND, "--shape_level", "nodes"], "--overlay_out" + NEEDS_EXPLAIN),
    (["--pose_colour", "{t}/o.csv", *COLOUR], "--pose_colour" + NEEDS_EXPLAIN),
    (["--combo_out", "{t}/o.csv", *COLOUR, *LIGAND, "--shape_level", "nodes"], "--combo_out" + NEEDS_EXPLAIN),
    (["--hotspots", "{t}/h.csv"], "--hotspots" + NEEDS_EXPLAIN),
    (["--modes", "3"], "--modes" + NEEDS_EXPLAIN),
    # the known ligand: its atoms and its features
    (["--explain", "3", "--pose_shape", "{t}/s.csv"], "--pose_shape needs --shape_ref FILE.pdb, the known ligand"),
    (["--explain", "5", "--overlay_out", "{t}/o.csv", "--shape_level", "nodes"], "--overlay_out needs --shape_ref FILE.pdb, the known ligand"),
    (["--explain", "5", "--combo_out", "{t}/o.csv", *COLOUR, "--shape_level", "nodes"], "--combo_out needs --shape_ref FILE.pdb, the known ligand"),
    (["--explain", "3", *LIGAND], "--shape_ref needs --pose_shape PATH or --overlay_out PATH"),
    (["--explain", "5", "--pose_colour", "{t}/o.csv"], "--pose_colour needs --colour_ref FILE.csv, the known ligand's features"),
    (["--explain", "5", "--combo_out", "{t}/o.csv", *LIGAND, "--shape_level", "nodes"], "--combo_out needs --colour_ref FILE.csv, the known ligand's features"),
    (["--explain", "5", *COLOUR], "--colour_ref needs --pose_colour PATH or --combo_out PATH"),
    (["--explain", "5", "--overlay_out", "{t}/o.csv", *LIGAND, "--shape_level", "nodes", "--overlay_iter", "65"], "--overlay_iter takes 0 to 64"),
    (["--explain", "5", "--combo_out", "{t}/o.csv", *COLOUR, *LIGAND, "--shape_level", "nodes", "--overlay_iter", "-1"], "--overlay_iter takes 0 to 64"),
    (["--explain", "5", "--overlay_out", "{t}/o.csv", *LIGAND, "--shape_level", "nodes", "--overlay_starts", "2"],
     "argument --overlay_starts: invalid choice: 2 (choose from 0, 4)"),
    (["--explain", "5", "--pose_colour", "{t}/o.csv", *COLOUR, "--colour_cover", "-1"], "--colour_cover takes a distance that is not negative"),
    (["--explain", "5", "--combo_out", "{t}/o.csv", *COLOUR, *LIGAND, "--shape_level", "nodes", "--combo_weight", "-1"],
     "--combo_weight takes a number that is not negative, or balanced"),
    (["--explain", "5", "--combo_out", "{t}/o.csv", *COLOUR, *LIGAND, "--shape_level", "nodes", "--combo_weight", "heavy"],
     "--combo_weight takes a number that is not negative, or balanced"),
    (["--explain", "3", "--pose_shape", "{t}/s.csv", *LIGAND, "--shape_level", "nodes", "--shape_cover", "-1"], "--shape_cover takes a distance that is not negative"),
    # the protein and the pose search
    (["--explain", "5", *POCKET], "--protein needs --clashes PATH, --refine_out PATH or --pose_search PATH"),
    (["--explain", "5", "--pose_search", "{t}/p.csv", "--pose_search_modes", "0"], "--pose_search_modes takes 1 to 8"),
    (["--explain", "5", "--pose_search", "{t}/p.csv", "--pose_search_modes", "9"], "--pose_search_modes takes 1 to 8"),
    (["--explain", "5", "--pose_search", "{t}/p.csv", "--pose_min_fraction", "1.5"], "--pose_min_fraction takes a number from 0 to 1"),
    (["--explain", "5", "--pose_search", "{t}/p.csv", "--pose_min_fraction", "nan"], "--pose_min_fraction takes a number from 0 to 1"),
    (["--explain", "5", "--pose_search", "{t}/p.csv", "--clash_tolerance", "nan"], "--clash_tolerance takes a number"),
    # atoms of a packed library that has no .atoms file
    (["--explain", "5", "--clashes", "{t}/c.csv", *POCKET], "--clash_level" + NO_ATOMS + "; or use --clash_level nodes)"),
    (["--explain", "5", *POCKET, "--refine_out", "{t}/r.csv"], "--clash_level" + NO_ATOMS + "; or use --clash_level nodes)"),
    (["--explain", "3", "--pose_shape", "{t}/s.csv", *LIGAND], "--shape_level" + NO_ATOMS + "; or use --shape_level nodes)"),
    (["--explain", "5", "--overlay_out", "{t}/o.csv", *LIGAND], "--shape_level" + NO_ATOMS + "; or use --shape_level nodes)"),
    (["--explain", "5", "--combo_out", "{t}/o.csv", *COLOUR, *LIGAND], "--shape_level" + NO_ATOMS + "; or use --shape_level nodes)"),
    (["--explain", "5", "--pose_search", "{t}/p.csv", *POCKET, "--pose_search_level", "atoms"], "--pose_search_level" + NO_ATOMS + ")"),
    # the clash check and the refinement
    (["--explain", "5", "--clashes", "{t}/c.csv", *POCKET, "--clash_level", "nodes", "--clash_tolerance", "inf"], "--clash_tolerance takes a number"),
    (["--explain", "5", *POCKET, "--refine_out", "{t}/r.csv", "--clash_level", "nodes", "--refine_restraint", "-1"], "--refine_restraint takes a number that is not negative"),
    (["--explain", "5", *POCKET, "--refine_out", "{t}/r.csv", "--clash_level", "nodes", "--refine_iter", "65"], "--refine_iter takes 0 to 64"),
    # diverse hits, modes, constraints, panel, saved hits
    (["--diverse", "0", "--diverse_out", "{t}/d.csv"], "--diverse takes a positive K"),
    (["--diverse", "5"], "--diverse needs --diverse_out PATH"),
    (["--diverse_out", "{t}/d.csv"], "--diverse_out / --diverse_pool need --diverse K"),
    (["--diverse_pool", "100"], "--diverse_out / --diverse_pool need --diverse K"),
    (["--diverse", "5", "--diverse_out", "{t}/d.csv", "--diverse_pool", "0"], "--diverse_pool takes 1 to 65536"),
    (["--diverse", "5", "--diverse_out", "{t}/d.csv", "--diverse_pool", "65537"], "--diverse_pool takes 1 to 65536"),
    (["--diverse", "5", "--diverse_out", "{t}/d.csv", "--diverse_threshold", "0"], "--diverse_threshold takes a similarity in (0, 1]"),
    (["--diverse", "5", "--diverse_out", "{t}/d.csv", "--diverse_threshold", "1.5"], "--diverse_threshold takes a similarity in (0, 1]"),
    (["--explain", "5", "--modes", "0"], "--modes takes 1 to 8"),
    (["--explain", "5", "--modes", "9"], "--modes takes 1 to 8"),
    (["--explain", "5", "--modes_out", "{t}/x.csv"], "--modes_out needs --modes M"),
    (["--require", "1"], "--require / --exclude need --constrained_out PATH"),
    (["--exclude", "1"], "--require / --exclude need --constrained_out PATH"),
    (["--constrained_out", "{t}/e.csv", "--constrained_k", "0"], "--constrained_k must be positive"),
    (["--require", "x", "--constrained_out", "{t}/e.csv"], "--require / --exclude take comma-separated model cluster indices"),
    (["--panel", "{g}/model_clustered21.pm"], "--panel needs --panel_out PATH"),
    (["--panel_out", "{t}/x.csv"], "--panel_out needs --panel MODEL"),
    (["--panel", "{g}/model_clustered21.pm", "--panel_out", "{t}/x.csv", "--panel_k", "0"], "--panel_k must be positive"),
    (["--save_top", "0", "{t}/top.pmxlib"], "--save_top takes a positive K and a path"),
    (["--save_top", "five", "{t}/top.pmxlib"], "--save_top takes a positive K and a path"),
    # validation and the ligand-based search
    (["--actives", "{t}/actives.txt"], "--actives FILE and --enrichment_out PATH go together"),
    (["--enrichment_out", "{t}/e.csv"], "--actives FILE and --enrichment_out PATH go together"),
    (["--enrichment_cut", "1,x"], "--enrichment_cut takes comma-separated percentages"),
    (["--actives", "{t}/actives.txt", "--enrichment_out", "{t}/e.csv", "--enrichment_cut", "1,200"], "--enrichment_cut takes 1 to 64 percentages between 0.0001 and 100"),
    (["--similar_to", "mol_12"], "--similar_to NAME and --similar_out PATH go together"),
    (["--similar_out", "{t}/x.csv"], "--similar_to NAME and --similar_out PATH go together"),
    (["--similar_to", "mol_12", "--similar_out", "{t}/x.csv", "--similar_k", "0"], "--similar_to takes up to 64 names, --similar_k 1 to 65536"),
    (["--bootstrap", "4097"], "--bootstrap takes 0 to 4096"),
    (["--bedroc_alpha", "0"], "--bedroc_alpha must be positive"),
    # refused once the model or the library has been read: still no GPU
    (["--explain", "5", "--clashes", "{t}/c.csv", "--clash_level", "nodes"],
     "--clashes: the model's pdbblock holds no ATOM / HETATM record ('SYNTHETIC 6OIM-LIKE'): give the protein with PocketAtoms.from_pdb (give it with --protein FILE.pdb)"),
    (["--actives", "{t}/actives.txt", "--enrichment_out", "{t}/x.csv"], "--actives {t}/actives.txt: 1 line(s) of the actives file match no ligand of the library: mol_999999"),
    (["--similar_to", "mol_999999", "--similar_out", "{t}/x.csv"], "--similar_to: 1 line(s) of --similar_to match no ligand of the library: mol_999999"),
    (["--similar_to", "mol_12", "--similar_to", "mol_12", "--similar_out", "{t}/x.csv"], "--similar_to: 1 name(s) of --similar_to are matched twice: mol_12"),
]

RUNNER = """
import contextlib, io, json, sys
from pharmaconet_amd.screening import main
results = []
for argv in json.load(open(sys.argv[1])):
    err, code = io.StringIO(), None
    with contextlib.redirect_stderr(err), contextlib.redirect_stdout(io.StringIO()):
        try:
            main(argv)
        except SystemExit as e:
            code = e.code
    results.append([code, (err.getvalue().splitlines() or [""])[-1], "torch" in sys.modules])
print(json.dumps(results))
"""


def run_cases(tmp_path):
    """Every case's (exit status, last line of stderr, whether torch got imported), from one fresh interpreter that runs them in turn."""
    shutil.copy(GOLDEN / "set_6oim_c5.pmxlib", tmp_path / "lib.pmxlib")
    from pharmaconet_amd.library import PackedLibrary

    n = len(PackedLibrary.load(tmp_path / "lib.pmxlib"))
    (tmp_path / "lib.pmxlib.names").write_text("\n".join(f"/data/mol_{i}.sdf" for i in range(n)))
    (tmp_path / "actives.txt").write_text("mol_1\nmol_999999\n")
    place = lambda s: s.replace("{t}", str(tmp_path)).replace("{g}", str(GOLDEN))  # noqa: E731
    (tmp_path / "cases.json").write_text(json.dumps([[place(a) for a in BASE + flags] for flags, _ in CASES]))
    done = subprocess.run([sys.executable, "-c", RUNNER, str(tmp_path / "cases.json")], cwd=REPO, capture_output=True, text=True, check=True)  # (-c: the package of this tree)
    return json.loads(done.stdout.splitlines()[-1]), place


def test_refused_command_lines_keep_their_messages(tmp_path):
    results, place = run_cases(tmp_path)
    assert len(results) == len(CASES)
    for (flags, message), (code, last, torch_loaded) in zip(CASES, results):
        assert code == 2, (flags, code, last)
        assert last == "scoring: error: " + place(message), flags
        assert not torch_loaded, flags
    assert not (tmp_path / "out.csv").exists()
