"""`python -m pharmaconet_amd.screening` - drop-in for the reference's `screening.py`.

Same flags (`screening.py:9-43`): `-p/--pharmacophore_model`, `-d/--library_dir`, `-o/--out`, `--cpus`, and the seven
type weights. `--library_dir` may be a directory of `.sdf` / `.mol2` files (perceived and packed on `--cpus` host
processes; needs OpenBabel like the reference) or a packed library file (`.pmxlib`, see
`pharmaconet_amd.library`) with an optional `<library>.names` text file giving one path per ligand.
Output: `path,score` CSV, best first, ties in library order (`screening.py:70-75`). Scoring runs on the GPU.
`--explain K --clashes PATH [--protein FILE.pdb]` checks the explained hits' poses against the protein's atoms (excluded volumes).
`--explain K --pose_shape PATH --shape_ref FILE.pdb` compares the explained hits' poses with a known ligand (Gaussian shape overlap).
`--explain K --overlay_out PATH --shape_ref FILE.pdb` overlays the explained hits on that ligand (a rigid maximisation of the overlap).
`--explain K --pose_colour PATH --colour_ref FILE.csv` compares the explained hits' typed nodes with that ligand's pharmacophore features.
`--explain K --combo_out PATH --shape_ref FILE.pdb --colour_ref FILE.csv` overlays the hits by shape and colour together.
`--explain K --refine_out PATH [--refine_restraint X] [--refine_iter N]` moves those poses out of the protein's atoms (restrained rigid-body refinement).
`--explain K --pose_fit PATH [--pose_fit_mode key|free]` scores those poses in place: the overlap of the posed pharmacophore nodes with the model's hotspots (with --refine_out also at the refined motion).
`--explain K --pose_search PATH [--pose_search_modes M] [--pose_min_fraction F] [--pose_search_level nodes|atoms]` poses every explained hit in the conformer and binding mode that fits the pocket.
`--panel MODEL ... --panel_out PATH` scores the best hits against other pockets; `--save_top K PATH` keeps them as a packed library.
`--actives FILE --enrichment_out PATH` validates the model retrospectively: the library's ligands named in FILE are the actives, the rest decoys.
`--similar_to NAME ... --similar_out PATH` lists the library's ligands most similar to the named ones by their own pharmacophore fingerprints.
"""

from __future__ import annotations

import argparse
import multiprocessing
import sys
from functools import cached_property
from pathlib import Path

import numpy as np

from .atoms import PackedAtoms, atoms_path
from .constants import TYPE_NAMES
from .library import PackedLibrary
from .pharmacophore_model import PharmacophoreModel


class Screening_ArgParser(argparse.ArgumentParser):
    def __init__(self):
        super().__init__("scoring")
        self.formatter_class = argparse.ArgumentDefaultsHelpFormatter
        cfg = self.add_argument_group("config")
        cfg.add_argument("-p", "--pharmacophore_model", type=str, required=True, help="path of pharmacophore model (.pm | .json)")
        cfg.add_argument("-d", "--library_dir", type=str, required=True, help="molecular library directory, or a packed .pmxlib file")
        cfg.add_argument("-o", "--out", type=str, required=True, help="result file path")
        cfg.add_argument("--cpus", type=int, default=1, help="host processes for reading / packing molecule files")
        cfg.add_argument("--explain", type=int, default=0, metavar="K", help="also explain the K best hits (best conformer and its cluster matches)")
        cfg.add_argument("--explain_out", type=str, default=None, help="CSV of the explained hits (default: <out>.explain.csv)")
        cfg.add_argument("--explain_nodes", type=str, default=None, metavar="PATH", help="with --explain K: CSV with one row per pharmacophore node of each explained hit and the node's share of the hit's best conformer maximum")
        cfg.add_argument("--poses", type=str, default=None, metavar="PATH", help="with --explain K: CSV with one row per explained hit and the rigid motion (rotation, translation) that puts its best conformer onto the matched pharmacophore points")
        cfg.add_argument("--clashes", type=str, default=None, metavar="PATH", help="with --explain K: CSV with one row per explained hit: its pose checked against the protein's heavy atoms (clashing points and pairs, deepest penetration, overlap, touched residues)")
        cfg.add_argument("--protein", type=str, default=None, metavar="FILE.pdb", help="with --clashes: the protein, in the model's frame (default: the protein the model carries)")
        cfg.add_argument("--clash_tolerance", type=float, default=0.5, metavar="T", help="with --clashes: overlap of two spheres, in Angstrom, that is not yet a clash")
        cfg.add_argument("--clash_level", choices=("nodes", "atoms"), default="atoms", help="with --clashes: check the hit's pharmacophore nodes, or its heavy atoms (of a library directory the hit files are read again; a packed library needs its .atoms file, which --save_top writes)")
        cfg.add_argument("--refine_out", type=str, default=None, metavar="PATH", help="with --explain K: CSV with one row per explained hit: its pose moved out of the protein's atoms by a restrained rigid-body refinement, checked before and after (uses --protein, --clash_tolerance and --clash_level)")
        cfg.add_argument("--pose_search", type=str, default=None, metavar="PATH", help="with --explain K: CSV with one row per explained hit: the conformer and binding mode, of all its conformers and their M best modes, whose fitted pharmacophore nodes do not clash with the protein (else the one of smallest overlap), with its motion (uses --protein and --clash_tolerance)")
        cfg.add_argument("--pose_search_modes", type=int, default=4, metavar="M", help="with --pose_search: binding modes searched per conformer (1 to 8)")
        cfg.add_argument("--pose_search_level", choices=("nodes", "atoms"), default="nodes", help="with --pose_search: choose on the fitted pharmacophore nodes, or on the hit's heavy atoms (the library's atom store: a library directory, or a .pmxlib with its .atoms file); clashing, overlap and clearance are then the atoms'")
        cfg.add_argument("--pose_min_fraction", type=float, default=0.0, metavar="F", help="with --pose_search: leave out poses whose match scores less than F (0 to 1) of the hit's best")
        cfg.add_argument("--pose_fit", type=str, default=None, metavar="PATH", help="with --explain K: CSV with one row per explained hit: how well the posed pharmacophore nodes sit on the model's hotspots (Gaussian overlap, the hotspot's radius as sigma); with --refine_out a second row per hit for the refined pose")
        cfg.add_argument("--pose_fit_mode", choices=("key", "free"), default="key", help="with --pose_fit: score the pairs of the hit's explaining match (key), or every hotspot of a type the node has (free)")
        cfg.add_argument("--pose_shape", type=str, default=None, metavar="PATH", help="with --explain K and --shape_ref: CSV with one row per explained hit: the Gaussian shape overlap of its pose with a known ligand (overlap volume, shape Tanimoto, the fractions of the reference and of the hit that are filled, nearest-atom distances both ways); with --refine_out a second row per hit for the refined pose")
        cfg.add_argument("--shape_ref", type=str, default=None, metavar="FILE.pdb", help="with --pose_shape: the known ligand, in the model's frame (its heavy atoms, Bondi radii)")
        cfg.add_argument("--shape_cover", type=float, default=2.0, metavar="D", help="with --pose_shape: an atom counts as covered when its nearest counterpart is closer than D Angstrom")
        cfg.add_argument("--overlay_out", type=str, default=None, metavar="PATH", help="with --explain K and --shape_ref: CSV with one row per explained hit: its best conformer overlaid on the known ligand (a rigid, local maximisation of the Gaussian shape overlap; no atom types): the shape Tanimoto before and after, how far the hit moved, and the motion")
        cfg.add_argument("--overlay_starts", type=int, choices=(0, 4), default=4, help="with --overlay_out: 4 runs each hit from the four motions that lay its inertial frame on the known ligand's and keeps the best; 0 starts from the hit's fitted pose")
        cfg.add_argument("--overlay_iter", type=int, default=32, metavar="N", help="with --overlay_out: at most N trial motions per start (0 to 64)")
        cfg.add_argument("--pose_colour", type=str, default=None, metavar="PATH", help="with --explain K and --colour_ref: CSV with one row per explained hit: the typed (colour) overlap of its posed pharmacophore nodes with a known ligand's features - matched nodes and features, the colour overlap, Tanimoto and fractions, and the overlap each type carries; points and types only, no directions")
        cfg.add_argument("--colour_ref", type=str, default=None, metavar="FILE.csv", help="with --pose_colour / --combo_out: the known ligand's pharmacophore features in the model's frame, lines type,x,y,z with type one of " + ", ".join(TYPE_NAMES))
        cfg.add_argument("--colour_cover", type=float, default=2.0, metavar="D", help="with --pose_colour: a node (a feature) counts as matched when its nearest partner of a shared type is closer than D Angstrom")
        cfg.add_argument("--combo_out", type=str, default=None, metavar="PATH", help="with --explain K, --shape_ref and --colour_ref: CSV with one row per explained hit: its best conformer overlaid on the known ligand by shape and colour together (a rigid, local maximisation of O_AB + W C_AB): the overlay CSV's columns and the colour Tanimoto before and after and the combo, the sum of the two Tanimotos")
        cfg.add_argument("--combo_weight", type=str, default="balanced", metavar="W|balanced", help="with --combo_out: the weight of the colour overlap against the shape overlap; balanced is O_BB / C_BB of the known ligand (derived, not calibrated)")
        cfg.add_argument("--shape_level", choices=("nodes", "atoms"), default="atoms", help="with --pose_shape / --overlay_out: compare the hit's pharmacophore nodes, or its heavy atoms (where they come from: as --clash_level)")
        cfg.add_argument("--refine_restraint", type=float, default=0.1, metavar="X", help="with --refine_out: the weight of the restraint that holds the pose near its fit (uncalibrated default)")
        cfg.add_argument("--refine_iter", type=int, default=32, metavar="N", help="with --refine_out: at most N trial motions per pose (0 to 64)")
        cfg.add_argument("--hotspots", type=str, default=None, metavar="PATH", help="with --explain K: CSV with one row per (explained hit, model node it has terms with): the node's share of the hit's best conformer maximum and whether the hit engages it")
        cfg.add_argument("--diverse", type=int, default=None, metavar="K", help="list the K first hits that are not the same binding mode again (leaders by interaction fingerprint, in rank order)")
        cfg.add_argument("--diverse_pool", type=int, default=None, metavar="P", help="best hits that --diverse looks at (default: max(8 K, 1024), at most 65536)")
        cfg.add_argument("--diverse_threshold", type=float, default=0.7, metavar="T", help="Tanimoto similarity from which a hit joins an earlier leader")
        cfg.add_argument("--diverse_out", type=str, default=None, metavar="PATH", help="CSV of the diverse hits (needed with --diverse)")
        cfg.add_argument("--modes", type=int, default=None, metavar="M", help="with --explain K: also list the M (1 to 8) best binding modes of each explained hit's best conformer")
        cfg.add_argument("--modes_out", type=str, default=None, metavar="PATH", help="CSV of the modes (default: <out>.modes.csv)")
        cfg.add_argument("--require", action="append", default=[], metavar="LIST", help="constrained matching: comma-separated model cluster indices, one of which a hit's match must hold (repeatable: one group each)")
        cfg.add_argument("--exclude", type=str, default=None, metavar="LIST", help="constrained matching: comma-separated model cluster indices that a hit's match must not hold")
        cfg.add_argument("--constrained_out", type=str, default=None, metavar="PATH", help="CSV of the best hits by constrained score (needed with --require / --exclude)")
        cfg.add_argument("--constrained_k", type=int, default=100, metavar="K", help="hits in --constrained_out")
        cfg.add_argument("--panel", action="append", default=[], metavar="MODEL", help="selectivity panel: another pharmacophore model (.pm | .json) the best hits are also scored against (repeatable)")
        cfg.add_argument("--panel_k", type=int, default=100, metavar="K", help="hits in --panel_out")
        cfg.add_argument("--panel_out", type=str, default=None, metavar="PATH", help="CSV of the K best hits with their score against every --panel model and the margin over the best of them (needed with --panel)")
        cfg.add_argument("--save_top", nargs=2, default=None, metavar=("K", "PATH"), help="keep the K best hits as a packed library PATH (.pmxlib, with PATH.names) that -d takes")
        cfg.add_argument("--actives", type=str, default=None, metavar="FILE", help="retrospective validation: a file with one ligand name per line (a name of the library, or its file stem) - the actives; every other ligand is a decoy")
        cfg.add_argument("--enrichment_out", type=str, default=None, metavar="PATH", help="CSV `metric,value,ci_low,ci_high` with AUROC, BEDROC and the enrichment factors (needed with --actives)")
        cfg.add_argument("--enrichment_cut", type=str, default="0.5,1,5", metavar="LIST", help="comma-separated cutoffs of the enrichment factors, in percent of the list")
        cfg.add_argument("--bedroc_alpha", type=float, default=20.0, metavar="A", help="BEDROC's alpha")
        cfg.add_argument("--bootstrap", type=int, default=0, metavar="B", help="bootstrap resamples behind the confidence intervals of --enrichment_out (0: none, at most 4096)")
        cfg.add_argument("--bootstrap_seed", type=int, default=0, metavar="S", help="seed of the bootstrap")
        cfg.add_argument("--similar_to", action="append", default=[], metavar="NAME", help="ligand-based search: a ligand of the library (a name of the library, or its file stem) whose neighbours by ligand pharmacophore fingerprint are listed (repeatable: up to 64 queries, fused by maximum)")
        cfg.add_argument("--similar_out", type=str, default=None, metavar="PATH", help="CSV `rank,path,similarity,<one column per query>` of the K most similar ligands (needed with --similar_to)")
        cfg.add_argument("--similar_k", type=int, default=100, metavar="K", help="ligands in --similar_out")
        par = self.add_argument_group("parameter")
        par.add_argument("--hydrophobic", type=float, default=1.0, help="weight for hydrophobic carbon")
        par.add_argument("--aromatic", type=float, default=4.0, help="weight for aromatic ring")
        par.add_argument("--hba", type=float, default=4.0, help="weight for hbond acceptor")
        par.add_argument("--hbd", type=float, default=4.0, help="weight for hbond donor")
        par.add_argument("--halogen", type=float, default=4.0, help="weight for halogen atom")
        par.add_argument("--anion", type=float, default=8.0, help="weight for anion")
        par.add_argument("--cation", type=float, default=8.0, help="weight for cation")


def _read_file(path: str):
    """One molecule file in a worker process: the toolkit parses it and answers the per-atom questions of perception
    (`ligand.toolkit_answers`); the conformer coordinates come with them. The rules and the packing run on the whole batch."""
    from .ligand import Ligand

    lig = Ligand.load_from_file(path)
    return lig.answers, lig.atom_positions


def load_library(library: Path, cpus: int, on_device: bool = False, with_atoms: bool = False):
    """(names, library) of a packed library file or of a directory of molecule files (screening.py:63-68). With `on_device` the records of a
    directory are made on the GPU (`pmx_pack_features_device`) and the library returned is device-resident; the host packer takes the batch if a
    molecule is beyond the device builder's fixed scratch, and always without `on_device` (library preparation on a host without a GPU).
    With `with_atoms` a third value: the library's atom store (`atoms.PackedAtoms`) - of a directory the molecules' heavy atoms, of a packed
    library what its `.atoms` file holds, None where there is no such file."""
    if library.is_file():
        lib = PackedLibrary.load(library)
        names_file = Path(str(library) + ".names")
        if names_file.exists():
            names = names_file.read_text().splitlines()
            if len(names) != len(lib):
                raise ValueError(f"{names_file}: {len(names)} names for {len(lib)} ligands")
        else:
            names = [f"{library}#{i}" for i in range(len(lib))]
        if with_atoms:
            store = PackedAtoms.load(atoms_path(library)) if atoms_path(library).is_file() else None
            if store is not None and len(store) != len(lib):
                raise ValueError(f"{atoms_path(library)}: atoms of {len(store)} ligands for a library of {len(lib)}")
            return names, lib, store
        return names, lib
    from .library import pack_features_native
    from .ligand import perceive_batch

    file_list = list(library.rglob("*.sdf")) + list(library.rglob("*.mol2"))  # screening.py:63-64
    print(f"find {len(file_list)} molecules")
    with multiprocessing.Pool(cpus) as pool:
        read = pool.map(_read_file, [str(f) for f in file_list])
    # features (ligand_utils.py:25-184) and records (LigandGraph, ligand.py:110-259) of all molecules at once, in native code
    flat = perceive_batch([a for a, _ in read], [p for _, p in read], threads=cpus)
    lib = status = None
    if on_device:
        from .engine import DeviceLibrary

        dlib = DeviceLibrary.from_features(flat, check=False)
        status = dlib.pack_status.cpu().numpy()
        if (status == 3).any():
            dlib.close()
        else:
            lib = dlib
    if lib is None:
        lib, status = pack_features_native(flat, threads=cpus)
    for f, st in zip(file_list, status):
        if st != 0:  # scored by the reference, not by this engine: reported, never silently dropped
            why = "outside the engine's structural limits (include/pmx.h)" if st == 1 else "feature graph the packer does not accept"
            print(f"warning: {f}: {why}; written with score nan", file=sys.stderr)
    if with_atoms:
        return [str(f) for f in file_list], lib, PackedAtoms.from_flat(flat, np.asarray(status) == 0)
    return [str(f) for f in file_list], lib


def write_csv(out: Path, names: list[str], scores: np.ndarray, status: np.ndarray | None = None) -> None:
    """`result.sort(key=score, reverse=True)` (stable) then `path,score` lines (screening.py:70-75).
    Scores print with Python's float repr of the value the GPU returned - the float64 mean of `graph_match.py:109` when `main` asks
    for it (`pmx_score_f64`), as the reference's CSV does. Ligands the engine could not score
    (`status != 0`: outside the structural limits of include/pmx.h) come last with score `nan`."""
    key = scores.astype(np.float64)
    bad = np.isnan(key) if status is None else (np.asarray(status) != 0)
    key = np.where(bad, -np.inf, key)
    order = np.lexsort((np.arange(len(scores)), -key))
    with open(out, "w") as w:
        w.write("path,score\n")
        for i in order:
            w.write(f"{names[i]},{'nan' if bad[i] else float(scores[i])}\n")
    if bad.any():
        print(f"warning: {int(bad.sum())} ligand(s) outside the engine's structural limits were not scored", file=sys.stderr)


def _best_hits(scores: np.ndarray, status: np.ndarray, k: int) -> list[int]:
    """The k best scored ligands in the order of the main CSV."""
    key = np.where(np.asarray(status) != 0, -np.inf, scores.astype(np.float64))
    return [int(i) for i in np.lexsort((np.arange(len(scores)), -key))[:k] if status[i] == 0]


class Hits:
    """The k explained hits of one run: what every side report of `--explain K` is written from. `main` makes it once, after the screen;
    each of `order`, `explanation`, `poses`, the hits' atoms, `clash_report` and `refined` is computed on first use and kept, so a run
    explains, fits, checks and refines its hits once however many reports it writes. `store` is a packed library's atom store (the hits'
    files are read again without it); `pocket`, `clash_level`, `tolerance`, `restraint` and `max_iter` are the run's one set of arguments
    of the clash check and the refinement. The level of a shape comparison is the caller's own (`atoms(level)`, `source(level)`)."""

    def __init__(self, names: list[str], scores: np.ndarray, status: np.ndarray, model, lib, weights, k: int, store: PackedAtoms | None = None, pocket=None,
                 clash_level: str = "nodes", tolerance: float = 0.5, restraint: float = 0.1, max_iter: int = 32):
        self.names, self.scores, self.status, self.model, self.lib, self.weights, self.k = names, scores, status, model, lib, weights, k
        self.store, self.pocket, self.clash_level, self.tolerance, self.restraint, self.max_iter = store, pocket, clash_level, tolerance, restraint, max_iter

    @cached_property
    def order(self) -> list[int]:
        """The hits as library indices, in the order of the main CSV: the command line's only ranking."""
        return _best_hits(self.scores, self.status, self.k)

    @cached_property
    def paths(self) -> list[str]:
        return [self.names[i] for i in self.order]

    @cached_property
    def explanation(self):
        from .engine import explain

        return explain(self.model, self.lib, self.order, weights=self.weights)

    @cached_property
    def poses(self):
        """The fit of every explained hit's best conformer under its explaining match (`engine.align`); `rows` are the explanation's rows."""
        return self.explanation.poses(self.model, self.lib, weights=self.weights)

    @cached_property
    def keys(self) -> list:
        return self.explanation._own_rows(None)[2]

    @cached_property
    def _atoms(self):
        if self.store is not None:
            return self.store
        from .ligand import Ligand

        return [Ligand.load_from_file(self.paths[int(row)]) for row in self.poses.rows]

    def atoms(self, level: str):
        """What the posed rows' methods take as `atoms` at `level`: None at `nodes`; at `atoms` the library's store, else the hits' files, read once."""
        return self._atoms if level == "atoms" else None

    def source(self, level: str) -> dict:
        """The keyword arguments that name the posed hits' points at `level` for the engine's row calls (`poses._pose_source`)."""
        from .engine import _pose_source

        return _pose_source(self.poses, "the explained hits", None, self.lib, self.atoms(level))[1]

    @cached_property
    def clash_report(self):
        return self.poses.clashes(self.pocket, self.lib, atoms=self.atoms(self.clash_level), tolerance=self.tolerance)

    @cached_property
    def refined(self):
        return self.poses.refine(self.pocket, self.lib, atoms=self.atoms(self.clash_level), tolerance=self.tolerance, restraint=self.restraint, max_iter=self.max_iter)


# ------------------------------------------------------------------------------------------------------------- row formats
# From result objects to text lines: nothing here calls the engine. `paths[i]` is the path of the explanation's row i.
MOTION_COLUMNS = ",".join(f"r{i}{j}" for i in range(3) for j in range(3)) + ",tx,ty,tz"
EXPLAIN_HEADER = "rank,path,score,best_conformer,conformer_max,matches"
MODES_HEADER = "rank,path,mode,mode_score,fraction_of_best,matches"
EXPLAIN_NODES_HEADER = "rank,index,path,conformer,node,node_types,ligand_cluster,model_cluster,node_score,share"
HOTSPOTS_HEADER = "rank,path,node,type,share,fraction,engaged"
POSES_HEADER = "rank,path,conformer,rmsd,rmsd_nodes,fitted_nodes," + MOTION_COLUMNS
POSE_SEARCH_HEADER = "rank,path,conformer,mode,passes,candidates,passing,mode_score,fraction_of_best,clashing,overlap,clearance,rmsd,rmsd_nodes,fitted_nodes," + MOTION_COLUMNS
CLASHES_HEADER = "rank,path,conformer,level,points,clashing,pairs,clearance,overlap,contacts,worst_point,worst_atom,residues"
REFINE_HEADER = ("rank,path,conformer,level,pairs_before,overlap_before,pairs_after,overlap_after,clearance_after,clashing_after,anchor_rmsd,angle_deg,shift,iterations,stop,"
                 + MOTION_COLUMNS)
POSE_FIT_HEADER = "rank,path,conformer,stage,fitted_nodes,pairs,in_place,passing,fit,ideal,fraction,best_fit,best_fraction,occupied_nodes"
POSE_SHAPE_HEADER = ("rank,path,conformer,stage,level,points,covered,reference_atoms,reference_covered,overlap,tanimoto,reference_fraction,fit_fraction,rms_to_reference,"
                     "rms_from_reference")
OVERLAY_HEADER = "rank,path,conformer,level,start,points,iterations,stop,tanimoto_start,tanimoto,overlap,reference_fraction,fit_fraction,angle_deg,shift," + MOTION_COLUMNS
POSE_COLOUR_HEADER = ("rank,path,conformer,stage,nodes,matched,reference_features,reference_matched,colour_overlap,colour_tanimoto,reference_fraction,fit_fraction,"
                      + ",".join(TYPE_NAMES))
COMBO_HEADER = OVERLAY_HEADER + ",colour_tanimoto_start,colour_tanimoto,combo"


def _num(*values) -> str:
    """Floats as the `repr` of the float64 the GPU returned, joined by commas."""
    return ",".join(repr(float(v)) for v in values)


def _motion(poses, r: int) -> str:
    """Row r's `MOTION_COLUMNS`: the rotation row by row, then the translation."""
    return _num(*poses.rotation[r].reshape(-1), *poses.translation[r])


def _hit(paths, al, r: int) -> str:
    """`rank,path,conformer` of row r of posed rows `al`: the rank and the path are those of the explanation's row behind it."""
    return f"{int(al.rows[r]) + 1},{paths[int(al.rows[r])]},{int(al.conformers[r])}"


def _matches(levels, match, types) -> str:
    """A key as `ligand cluster->model cluster:type` pairs; levels matched to None are left out."""
    return " ".join(f"{lc}->{int(m)}:{types[int(m)]}" for lc, m in zip(levels, match) if m >= 0)


def _write(out: Path, header: str, lines) -> None:
    with open(out, "w") as w:
        w.write(header + "\n")
        w.writelines(line + "\n" for line in lines)


def explain_rows(paths, scores, ex, types):
    """`scores[i]` is the main CSV's score of the explanation's row i; `types` the model's cluster types."""
    for r, path in enumerate(paths):
        c = int(ex.best_conformer[r])
        yield f"{r + 1},{path},{_num(scores[r])},{c},{_num(ex.conf_max[r][c])},{_matches(ex.levels[r], ex.match[r][c], types) if c >= 0 else ''}"


def modes_rows(paths, ms, types):
    for r, path in enumerate(paths):
        c = int(ms.best_conformer[r])
        for m in range(int(ms.count(r)[c]) if c >= 0 and ms.values[r].shape[1] else 0):
            v = float(ms.values[r][m, c])
            yield f"{r + 1},{path},{m},{_num(v, v / float(ms.values[r][0, c]))},{_matches(ms.levels[r], ms.match[r][m, c], types)}"


def explain_nodes_rows(paths, order, ex, at, records):
    """`order[i]` is the library index of the explanation's row i, `records[r]` the unpacked record behind the attribution's row r."""
    for r, row in enumerate(at.rows):
        rec, c = records[r], int(at.conformers[r])
        matched = {int(lc): int(m) for lc, m in zip(ex.levels[row], ex.match[row][c]) if m >= 0}
        total = float(at.total[r])
        for u, share in enumerate(at.node[r]):
            lc = int(np.searchsorted(rec["cluster_end"], u, side="right"))
            tm = int(rec["typemask"][u])
            types = "|".join(TYPE_NAMES[t] for t in range(len(TYPE_NAMES)) if tm >> t & 1)
            yield f"{int(row) + 1},{order[int(row)]},{paths[int(row)]},{c},{u},{types},{lc},{matched.get(lc, '')},{_num(share, float(share) / total if total > 0 else 0.0)}"


def hotspots_rows(paths, hs, node_type):
    for r, row in enumerate(hs.rows):
        total = float(hs.total[r])
        engaged = set(hs.nodes(r).tolist())
        for m in np.flatnonzero(hs.terms[r] > 0):
            share = float(hs.share[r][m])
            yield f"{int(row) + 1},{paths[int(row)]},{int(m)},{TYPE_NAMES[int(node_type[m])]},{_num(share, share / total if total > 0 else 0.0)},{int(int(m) in engaged)}"


def poses_rows(paths, al):
    for r in range(len(al.rows)):
        yield f"{_hit(paths, al, r)},{_num(al.rmsd[r], al.rmsd_nodes[r])},{int(al.n_nodes[r])},{_motion(al, r)}"


def pose_search_rows(paths, ps, al, rep):
    """`al` and `rep` are the search's own alignment and clash report: one row per hit, in the hits' order."""
    for r in range(len(ps.conformer)):
        yield (f"{r + 1},{paths[r]},{int(ps.conformer[r])},{int(ps.mode[r])},{int(ps.passes[r])},{int(ps.n_candidates[r])},{int(ps.n_passing[r])},{_num(ps.value[r], ps.fraction[r])},"
               f"{int(rep.n_clashing[r])},{_num(rep.overlap[r], rep.clearance[r], al.rmsd[r], al.rmsd_nodes[r])},{int(al.n_nodes[r])},{_motion(al, r)}")


def clashes_rows(paths, al, rep, level: str, pocket):
    for r in range(len(al.rows)):
        yield (f"{_hit(paths, al, r)},{level},{int(rep.n_points[r])},{int(rep.n_clashing[r])},{int(rep.n_pairs[r])},{_num(rep.clearance[r], rep.overlap[r])},{int(rep.n_contacts[r])},"
               f"{int(rep.worst[r, 0])},{rep.atom_label(r, pocket)},{';'.join(rep.residues(r, pocket))}")


def refine_rows(paths, al, before, ref, after, level: str):
    for r in range(len(al.rows)):
        yield (f"{_hit(paths, al, r)},{level},{int(before.n_pairs[r])},{_num(before.overlap[r])},{int(after.n_pairs[r])},{_num(after.overlap[r], after.clearance[r])},"
               f"{int(after.n_clashing[r])},{_num(ref.anchor_rmsd[r], np.degrees(ref.angle[r]), ref.shift[r])},{int(ref.iterations[r])},{int(ref.stop[r])},{_motion(ref, r)}")


def pose_fit_rows(paths, al, stages):
    """`stages`: (stage name, `PoseFit`) pairs; a hit's rows are together."""
    for r in range(len(al.rows)):
        for stage, pf in stages:
            yield (f"{_hit(paths, al, r)},{stage},{int(pf.n_nodes[r])},{int(pf.n_pairs[r])},{int(pf.n_in_place[r])},{int(pf.n_passing[r])},"
                   f"{_num(pf.fit[r], pf.ideal[r], pf.fraction[r], pf.best_fit[r], pf.best_fraction[r])},{';'.join(str(int(m)) for m in pf.occupied(r))}")


def pose_shape_rows(paths, al, stages, level: str, n_reference: int):
    """`stages`: (stage name, `ShapeReport`) pairs; a hit's rows are together."""
    for r in range(len(al.rows)):
        for stage, sh in stages:
            yield (f"{_hit(paths, al, r)},{stage},{level},{int(sh.n_points[r])},{int(sh.n_covered[r])},{n_reference},{int(sh.n_reference_covered[r])},"
                   f"{_num(sh.overlap[r], sh.tanimoto[r], sh.reference_fraction[r], sh.fit_fraction[r], sh.rms_to_reference[r], sh.rms_from_reference[r])}")


def overlay_rows(paths, al, ov, level: str, combo: bool = False):
    """The overlay CSV's rows of a `ShapeOverlay`; with `combo` those of a `ComboOverlay`, which end on its three colour columns."""
    with np.errstate(all="ignore"):
        ref_fraction = ov.overlap / ov.reference_overlap
        fit_fraction = np.where(ov.self_overlap == 0.0, 0.0, ov.overlap / np.where(ov.self_overlap == 0.0, 1.0, ov.self_overlap))
    for r in range(len(al.rows)):
        yield (f"{_hit(paths, al, r)},{level},{int(ov.start[r])},{int(ov.n_points[r])},{int(ov.iterations[r])},{int(ov.stop[r])},"
               f"{_num(ov.tanimoto_start[r], ov.tanimoto[r], ov.overlap[r], ref_fraction[r], fit_fraction[r], np.degrees(ov.angle[r]), ov.shift[r])},{_motion(ov, r)}"
               + (f",{_num(ov.colour_tanimoto_start[r], ov.colour_tanimoto[r], ov.combo[r])}" if combo else ""))


def pose_colour_rows(paths, al, rep, n_reference: int):
    for r in range(len(al.rows)):
        yield (f"{_hit(paths, al, r)},fit,{int(rep.n_nodes[r])},{int(rep.n_matched[r])},{n_reference},{int(rep.n_reference_matched[r])},"
               f"{_num(rep.overlap[r], rep.tanimoto[r], rep.reference_fraction[r], rep.fit_fraction[r], *rep.type_overlap[r])}")


# ------------------------------------------------------------------------------------------------------------- the side reports
def write_explain_csv(out: Path, hits: Hits) -> None:
    """The k best hits of a screen, in the order of the main CSV, with the best conformer, its maximum and its matched pairs
    `ligand cluster -> model cluster:type` (ligand clusters as indices of the record's priority-ordered cluster list, model clusters as
    indices of `model.node_clusters`; levels matched to None are left out): `engine.explain` on those k ligands only."""
    _write(out, EXPLAIN_HEADER, explain_rows(hits.paths, [hits.scores[i] for i in hits.order], hits.explanation, hits.model.flat.cluster_type))


def write_modes_csv(out: Path, hits: Hits, modes: int) -> None:
    """One row per (hit, mode) of the k best hits, in the order of the explain CSV: the `modes` best leaves of the hit's best conformer
    (`engine.explain_modes`), best first - the leaf's total, the total as a fraction of mode 0's (the explain CSV's conformer_max), and
    its matched pairs in the explain CSV's format. Modes the conformer does not have are left out."""
    from .engine import explain_modes

    ms = explain_modes(hits.model, hits.lib, hits.order, modes=modes, weights=hits.weights)
    _write(out, MODES_HEADER, modes_rows(hits.paths, ms, hits.model.flat.cluster_type))


def _record_of(lib, i: int) -> dict:
    """Record i of a packed library, or of a device-resident one of any origin (its buffers are read back for that record)."""
    if isinstance(lib, PackedLibrary):
        return lib.unpack(i)
    offsets, data = lib.buffers()
    lo, hi = (int(x) for x in offsets[i : i + 2].cpu())
    return PackedLibrary.from_records([data[lo:hi].cpu().numpy().tobytes()]).unpack(0)


def write_explain_nodes_csv(out: Path, hits: Hits) -> None:
    """One row per (hit, node) of the k best hits, in the order of the main CSV: the node's index in the packed record, its types, its
    ligand cluster, the model cluster that cluster is matched to in the explaining leaf of the hit's best conformer (empty for None and
    for clusters outside the tree), the node's share of that conformer's maximum (`engine.attribute`) and the share as a fraction of it."""
    at = hits.explanation.attribution(hits.model, hits.lib, weights=hits.weights)
    records = [_record_of(hits.lib, hits.order[int(row)]) for row in at.rows]
    _write(out, EXPLAIN_NODES_HEADER, explain_nodes_rows(hits.paths, hits.order, hits.explanation, at, records))


def write_hotspots_csv(out: Path, hits: Hits) -> None:
    """One row per (hit, model node the hit has terms with) of the k best hits, in the order of the explain CSV: the node's index in the
    model, its type, its share of the hit's best conformer maximum (`engine.hotspots`), the share as a fraction of it, and 1 where the
    hit engages the node (the node's bit of the hit's interaction fingerprint)."""
    hs = hits.explanation.hotspots(hits.model, hits.lib, weights=hits.weights)
    _write(out, HOTSPOTS_HEADER, hotspots_rows(hits.paths, hs, hits.model.flat.node_type))


def write_poses_csv(out: Path, hits: Hits) -> None:
    """One row per hit of the k best, in the order of the explain CSV: the fit of the hit's best conformer under its explaining match
    (`engine.align`) - the two RMSDs, the fitted nodes and the motion `x -> R x + t` (R row by row) that poses the conformer in the
    pocket. Every number is the `repr` of the float64 the GPU returned."""
    _write(out, POSES_HEADER, poses_rows(hits.paths, hits.poses))


def write_pose_search_csv(out: Path, hits: Hits, pocket, tolerance: float, modes: int, min_fraction: float, store: PackedAtoms | None = None) -> None:
    """One row per hit of the k best, in the order of the poses CSV: the hit posed where `engine.pose_search` puts it - of all its conformers
    under their `modes` best binding modes the best-scoring one whose fitted pharmacophore nodes do not clash with the protein, else the
    one of smallest overlap. The conformer and mode (-1 and -1 for a hit without any pose), whether it passes, how many candidates there
    were and how many passed, the mode's leaf total and its share of the hit's best, the clash check and the fit of the chosen pose, and
    the motion as the poses CSV has it. Every number is the `repr` of the float64 the GPU returned. With `store`, the library's atom store, the
    search chooses on the hits' heavy atoms (`--pose_search_level atoms`): the same columns, the clash values then being the atoms'."""
    from .engine import pose_search

    ps = pose_search(hits.model, hits.lib, pocket, hits.order, modes=modes, weights=hits.weights, min_fraction=min_fraction, tolerance=tolerance, atoms=store)
    _write(out, POSE_SEARCH_HEADER, pose_search_rows(hits.paths, ps, ps.alignment(), ps.report()))


def write_clashes_csv(out: Path, hits: Hits) -> None:
    """One row per hit of the k best, in the order of the poses CSV: the pose of the hit's best conformer (`engine.align`) checked against the
    protein's heavy atoms (`engine.clashes`) - at level `nodes` the hit's pharmacophore nodes, at level `atoms` the heavy atoms of the hit's
    file, read again. Points, clashing points, clashing pairs, the deepest penetration (negative: the clearance), the overlap, the points
    within contact distance, the worst pair's point and protein atom, and the touched residues joined by `;`."""
    _write(out, CLASHES_HEADER, clashes_rows(hits.paths, hits.poses, hits.clash_report, hits.clash_level, hits.pocket))


def write_refine_csv(out: Path, hits: Hits) -> None:
    """One row per hit of the k best, in the order of the poses CSV: the pose of the hit's best conformer (`engine.align`) moved out of the
    protein's heavy atoms (`engine.refine`) - the hit's pharmacophore nodes at level `nodes`, the heavy atoms of its file at level `atoms` -
    with the check (`engine.clashes`) before and after: clashing pairs and overlap before; pairs, overlap, the deepest penetration and the
    clashing points after; how far the anchors moved (rmsd), the net rotation in degrees, the centroid's shift, the trial motions taken and
    why they ended (`RefinedPoses.stop`); the refined rotation, row-major, and translation. A pose that is not OK has nan and stop -1."""
    after = hits.refined.clashes(hits.pocket, hits.lib, atoms=hits.atoms(hits.clash_level), tolerance=hits.tolerance)
    _write(out, REFINE_HEADER, refine_rows(hits.paths, hits.poses, hits.clash_report, hits.refined, after, hits.clash_level))


def write_pose_fit_csv(out: Path, hits: Hits, mode: str, refined: bool = False) -> None:
    """One row per hit of the k best, in the order of the poses CSV, with stage `fit`: the pose of the hit's best conformer (`engine.align`)
    scored in place (`engine.pose_fit`) - in mode `key` over the pairs of the explaining match, in mode `free` over every hotspot of a type
    the node has. Nodes with a pair, pairs, nodes in place, passing pairs, the fit, its ideal and their ratio, the same over each node's
    nearest hotspot, and the occupied model nodes joined by `;`. With `refined` a second row per hit, stage `refined`, for the motion the
    run's refinement (`Hits.refined`) ends at. Every float is the `repr` of the float64 the GPU returned."""
    keys = hits.keys if mode == "key" else None
    stages = [("fit", hits.poses)] + ([("refined", hits.refined)] if refined else [])
    _write(out, POSE_FIT_HEADER, pose_fit_rows(hits.paths, hits.poses, [(stage, p.pose_fit(hits.model, hits.lib, keys=keys, weights=hits.weights)) for stage, p in stages]))


def write_pose_shape_csv(out: Path, hits: Hits, reference, level: str, cover: float, refined: bool = False) -> None:
    """One row per hit of the k best, in the order of the poses CSV, with stage `fit`: the pose of the hit's best conformer (`engine.align`)
    compared with the known ligand `reference` (`engine.shape`) - at level `nodes` the hit's pharmacophore nodes, at level `atoms` its heavy
    atoms, from where the clashes CSV takes them. Points and the points within `cover` of a reference atom, the reference's atoms and
    those within `cover` of a point, the overlap volume, the shape Tanimoto, the fraction of the reference that is filled and of the hit that
    lies inside it, and the root mean square nearest-atom distance both ways. With `refined` a second row per hit, stage `refined`, for the
    motion the run's refinement ends at (it moved the points of the clash level; the comparison is at `level`). Every float is the `repr` of
    the float64 the GPU returned."""
    stages = [("fit", hits.poses)] + ([("refined", hits.refined)] if refined else [])
    _write(out, POSE_SHAPE_HEADER, pose_shape_rows(hits.paths, hits.poses, [(stage, p.shape(reference, hits.lib, atoms=hits.atoms(level), cover=cover)) for stage, p in stages],
                                                   level, len(reference)))


def _start_motion(hits: Hits, starts: int) -> dict:
    """Where an overlay starts: with `starts` 4 from the inertial starts (no motion is given), with 0 from the hits' fitted poses."""
    return {} if starts else dict(rotation=hits.poses.rotation, translation=hits.poses.translation)


def write_overlay_csv(out: Path, hits: Hits, reference, level: str, starts: int, max_iter: int) -> None:
    """One row per hit of the k best, in the order of the poses CSV: the hit's best conformer overlaid on the known ligand `reference`
    (`engine.overlay`) - at level `nodes` its pharmacophore nodes, at level `atoms` its heavy atoms, from where the pose-shape CSV takes
    them. With `starts` 4 the hit is run from the four inertial starts and `start` says which was kept; with 0 it is run from its fitted
    pose (`engine.align`) and `start` is -1. The shape Tanimoto at the start and at the end, the overlap volume there, the fraction of the
    reference that is filled and of the hit that lies inside it, the net rotation in degrees and the centroid's shift from the start, and
    the motion. Every float is the `repr` of the float64 the GPU returned (the two fractions and the degrees are formed from them)."""
    from .engine import overlay

    ov = overlay(reference, starts=starts, max_iter=max_iter, **_start_motion(hits, starts), **hits.source(level))
    _write(out, OVERLAY_HEADER, overlay_rows(hits.paths, hits.poses, ov, level))


def write_pose_colour_csv(out: Path, hits: Hits, reference, cover: float) -> None:
    """One row per hit of the k best, in the order of the poses CSV, with stage `fit`: the pharmacophore nodes of the hit's best conformer
    under its fitted pose (`engine.align`) compared with the known ligand's typed features `reference` (`engine.colour`). Nodes and the
    nodes with a partner of a shared type within `cover`, the reference's features and those reproduced, the colour overlap, its Tanimoto,
    the fraction of the reference that is reproduced and of the hit that lies on it, and the overlap each type carries. Every float is the
    `repr` of the float64 the GPU returned."""
    from .engine import colour_of

    _write(out, POSE_COLOUR_HEADER, pose_colour_rows(hits.paths, hits.poses, colour_of(hits.poses, reference, hits.lib, cover=cover), len(reference)))


def write_combo_csv(out: Path, hits: Hits, reference, colour, colour_weight, level: str, starts: int, max_iter: int) -> None:
    """One row per hit of the k best, in the order of the poses CSV: the hit's best conformer overlaid on the known ligand by shape and
    colour together (`engine.combo_overlay`; `reference` its atoms, `colour` its typed features). The columns of the overlay CSV - the
    shape points at level `nodes` the hit's pharmacophore nodes, at level `atoms` its heavy atoms - and the colour Tanimoto at the start
    and at the end and the combo at the end, the sum of the two Tanimotos. The typed points are always the hit's nodes."""
    from .engine import combo_overlay

    al = hits.poses
    rows = dict(dict(library=hits.lib, indices=al.indices, conformers=al.conformers), **hits.source(level))  # (the records always: their nodes carry the types)
    ov = combo_overlay(reference, colour=colour, colour_weight=colour_weight, starts=starts, max_iter=max_iter, **_start_motion(hits, starts), **rows)
    _write(out, COMBO_HEADER, overlay_rows(hits.paths, al, ov, level, combo=True))


# (flag, the flag that holds the path, writer, the writer's further arguments from the run `s`: the parsed flags and what `main` read for them) of every
# side report of the explained hits, in the order their files are written
SIDE_REPORTS = (
    ("explain_nodes", "explain_nodes", write_explain_nodes_csv, lambda s: ()),
    ("poses", "poses", write_poses_csv, lambda s: ()),
    ("clashes", "clashes", write_clashes_csv, lambda s: ()),
    ("refine_out", "refine_out", write_refine_csv, lambda s: ()),
    ("pose_fit", "pose_fit", write_pose_fit_csv, lambda s: (s.pose_fit_mode, bool(s.refine_out))),
    ("pose_shape", "pose_shape", write_pose_shape_csv, lambda s: (s.shape_reference, s.shape_level, s.shape_cover, bool(s.refine_out))),
    ("overlay_out", "overlay_out", write_overlay_csv, lambda s: (s.shape_reference, s.shape_level, s.overlay_starts, s.overlay_iter)),
    ("pose_colour", "pose_colour", write_pose_colour_csv, lambda s: (s.colour_reference, s.colour_cover)),
    ("combo_out", "combo_out", write_combo_csv, lambda s: (s.shape_reference, s.colour_reference, s.colour_weight, s.shape_level, s.overlay_starts, s.overlay_iter)),
    ("pose_search", "pose_search", write_pose_search_csv, lambda s: (s.pocket, s.clash_tolerance, s.pose_search_modes, s.pose_min_fraction, s.search_store)),
    ("hotspots", "hotspots", write_hotspots_csv, lambda s: ()),
    ("modes", "modes_out", write_modes_csv, lambda s: (s.modes,)),
)


def _asked(args, flag: str) -> bool:
    """Whether the run asks for the side report behind `flag`: a path that is not empty, or --modes' M (0 included: refused later)."""
    value = getattr(args, flag)
    return value is not None and value != ""


def main(argv=None) -> None:
    parser = Screening_ArgParser()
    args = parser.parse_args(argv)
    for flag, *_ in SIDE_REPORTS:
        if _asked(args, flag) and args.explain <= 0:
            parser.error(f"--{flag} needs --explain K")
    if args.pose_shape and not args.shape_ref:
        parser.error("--pose_shape needs --shape_ref FILE.pdb, the known ligand")
    if args.overlay_out and not args.shape_ref:
        parser.error("--overlay_out needs --shape_ref FILE.pdb, the known ligand")
    if args.overlay_out and not 0 <= args.overlay_iter <= 64:
        parser.error("--overlay_iter takes 0 to 64")
    if args.shape_ref and not (args.pose_shape or args.overlay_out or args.combo_out):
        parser.error("--shape_ref needs --pose_shape PATH or --overlay_out PATH")
    if (args.pose_colour or args.combo_out) and not args.colour_ref:
        parser.error(f"{'--pose_colour' if args.pose_colour else '--combo_out'} needs --colour_ref FILE.csv, the known ligand's features")
    if args.combo_out and not args.shape_ref:
        parser.error("--combo_out needs --shape_ref FILE.pdb, the known ligand")
    if args.colour_ref and not (args.pose_colour or args.combo_out):
        parser.error("--colour_ref needs --pose_colour PATH or --combo_out PATH")
    if args.pose_colour and not (np.isfinite(args.colour_cover) and args.colour_cover >= 0):
        parser.error("--colour_cover takes a distance that is not negative")
    if args.combo_out and not 0 <= args.overlay_iter <= 64:
        parser.error("--overlay_iter takes 0 to 64")
    args.colour_weight = "balanced"
    if args.combo_out and args.combo_weight != "balanced":
        try:
            args.colour_weight = float(args.combo_weight)
        except ValueError:
            args.colour_weight = float("nan")
        if not (np.isfinite(args.colour_weight) and args.colour_weight >= 0):
            parser.error("--combo_weight takes a number that is not negative, or balanced")
    if args.pose_shape and not (np.isfinite(args.shape_cover) and args.shape_cover >= 0):
        parser.error("--shape_cover takes a distance that is not negative")
    if not (args.clashes or args.refine_out or args.pose_search) and args.protein:
        parser.error("--protein needs --clashes PATH, --refine_out PATH or --pose_search PATH")
    if args.pose_search and not 1 <= args.pose_search_modes <= 8:
        parser.error("--pose_search_modes takes 1 to 8")
    if args.pose_search and not 0.0 <= args.pose_min_fraction <= 1.0:
        parser.error("--pose_min_fraction takes a number from 0 to 1")
    if args.pose_search and not np.isfinite(args.clash_tolerance):
        parser.error("--clash_tolerance takes a number")
    packed_without_atoms = (Path(args.library_dir).is_file() or args.library_dir.endswith(".pmxlib")) and not atoms_path(args.library_dir).is_file()
    if (args.clashes or args.refine_out) and args.clash_level == "atoms" and packed_without_atoms:
        parser.error(f"--clash_level atoms takes the hits' atoms from {atoms_path(args.library_dir)}, which does not exist (--save_top writes it from a library directory; "
                     "or use --clash_level nodes)")
    if (args.pose_shape or args.overlay_out or args.combo_out) and args.shape_level == "atoms" and packed_without_atoms:
        parser.error(f"--shape_level atoms takes the hits' atoms from {atoms_path(args.library_dir)}, which does not exist (--save_top writes it from a library directory; "
                     "or use --shape_level nodes)")
    if args.pose_search and args.pose_search_level == "atoms" and packed_without_atoms:
        parser.error(f"--pose_search_level atoms takes the hits' atoms from {atoms_path(args.library_dir)}, which does not exist (--save_top writes it from a library directory)")
    if (args.clashes or args.refine_out) and not np.isfinite(args.clash_tolerance):
        parser.error("--clash_tolerance takes a number")
    if args.refine_out and not (np.isfinite(args.refine_restraint) and args.refine_restraint >= 0):
        parser.error("--refine_restraint takes a number that is not negative")
    if args.refine_out and not 0 <= args.refine_iter <= 64:
        parser.error("--refine_iter takes 0 to 64")
    if args.diverse is not None and args.diverse <= 0:
        parser.error("--diverse takes a positive K")
    if args.diverse is not None and not args.diverse_out:
        parser.error("--diverse needs --diverse_out PATH")
    if args.diverse is None and (args.diverse_out or args.diverse_pool is not None):
        parser.error("--diverse_out / --diverse_pool need --diverse K")
    if args.diverse_pool is not None and not 1 <= args.diverse_pool <= 65536:
        parser.error("--diverse_pool takes 1 to 65536")
    if not 0.0 < args.diverse_threshold <= 1.0:
        parser.error("--diverse_threshold takes a similarity in (0, 1]")
    if args.modes is not None and not 1 <= args.modes <= 8:
        parser.error("--modes takes 1 to 8")
    if args.modes_out and args.modes is None:
        parser.error("--modes_out needs --modes M")
    if (args.require or args.exclude is not None) and not args.constrained_out:
        parser.error("--require / --exclude need --constrained_out PATH")
    if args.constrained_out and args.constrained_k <= 0:
        parser.error("--constrained_k must be positive")
    if args.panel and not args.panel_out:
        parser.error("--panel needs --panel_out PATH")
    if args.panel_out and not args.panel:
        parser.error("--panel_out needs --panel MODEL")
    if args.panel_out and args.panel_k <= 0:
        parser.error("--panel_k must be positive")
    if args.save_top:
        try:
            save_k = int(args.save_top[0])
        except ValueError:
            save_k = 0
        if save_k <= 0:
            parser.error("--save_top takes a positive K and a path")
    if bool(args.actives) != bool(args.enrichment_out):
        parser.error("--actives FILE and --enrichment_out PATH go together")
    try:
        enrichment_cut = [float(v) / 100.0 for v in args.enrichment_cut.split(",")]
    except ValueError:
        parser.error("--enrichment_cut takes comma-separated percentages")
    if args.actives and (not enrichment_cut or len(enrichment_cut) > 64 or any(not 1e-6 <= c <= 1.0 for c in enrichment_cut)):
        parser.error("--enrichment_cut takes 1 to 64 percentages between 0.0001 and 100")
    if bool(args.similar_to) != bool(args.similar_out):
        parser.error("--similar_to NAME and --similar_out PATH go together")
    if args.similar_to and not (len(args.similar_to) <= 64 and 0 < args.similar_k <= 65536):
        parser.error("--similar_to takes up to 64 names, --similar_k 1 to 65536")
    if not 0 <= args.bootstrap <= 4096:
        parser.error("--bootstrap takes 0 to 4096")
    if not args.bedroc_alpha > 0:
        parser.error("--bedroc_alpha must be positive")
    try:
        require = [[int(v) for v in g.split(",")] for g in args.require]
        exclude = [int(v) for v in args.exclude.split(",")] if args.exclude else []
    except ValueError:
        parser.error("--require / --exclude take comma-separated model cluster indices")
    model = PharmacophoreModel.load(args.pharmacophore_model)
    weight = dict(
        Cation=args.cation,
        Anion=args.anion,
        Aromatic=args.aromatic,
        HBond_donor=args.hbd,
        HBond_acceptor=args.hba,
        Halogen=args.halogen,
        Hydrophobic=args.hydrophobic,
    )
    args.pocket = args.shape_reference = args.colour_reference = None
    if args.clashes or args.refine_out or args.pose_search:  # (before the screen: a model without a protein should not cost a pass)
        from .pocket import PocketAtoms

        try:
            args.pocket = PocketAtoms.from_pdb(Path(args.protein), centers=model.node_centers) if args.protein else model.pocket_atoms()
        except (OSError, ValueError) as e:
            parser.error(f"{'--clashes' if args.clashes else '--refine_out' if args.refine_out else '--pose_search'}: {e}" + ("" if args.protein else " (give it with --protein FILE.pdb)"))
    if args.pose_colour or args.combo_out:
        from .shape import ColourFeatures

        try:
            args.colour_reference = ColourFeatures.from_csv(Path(args.colour_ref))
        except (OSError, ValueError) as e:
            parser.error(f"--colour_ref {args.colour_ref}: {e}")
    if args.pose_shape or args.overlay_out or args.combo_out:  # (before the screen: a reference that cannot be read should not cost a pass)
        from .shape import ReferenceLigand

        try:
            args.shape_reference = ReferenceLigand.from_pdb(Path(args.shape_ref))
        except (OSError, ValueError) as e:
            parser.error(f"--shape_ref {args.shape_ref}: {e}")
    # the library's atom store: the check of a packed library's atoms, the atom-level search, and what --save_top keeps next to the records
    packed = Path(args.library_dir).is_file()
    atom_search = bool(args.pose_search) and args.pose_search_level == "atoms"
    if (atom_search or args.save_top or (packed and (args.clashes or args.refine_out) and args.clash_level == "atoms")
            or (packed and (args.pose_shape or args.overlay_out or args.combo_out) and args.shape_level == "atoms")):
        names, lib, store = load_library(Path(args.library_dir), args.cpus, on_device=True, with_atoms=True)
    else:
        (names, lib), store = load_library(Path(args.library_dir), args.cpus, on_device=True), None
    args.search_store = store if atom_search else None
    if args.actives:  # (before the screen: a name that matches nothing should not cost a pass)
        from .validation import match_actives

        try:
            labels = match_actives(Path(args.actives).read_text().splitlines(), names)
        except ValueError as e:
            parser.error(f"--actives {args.actives}: {e}")
    if args.similar_to:
        from .validation import match_actives

        try:
            match_actives(args.similar_to, names)  # (every name once, and each a ligand of the library)
            queries = [int(np.flatnonzero(match_actives([q], names))[0]) for q in args.similar_to]
        except ValueError as e:
            parser.error(f"--similar_to: {str(e).replace('the actives file', '--similar_to')}")
    result = model.screen(lib, weights=weight, float64=True)  # (the reference writes the float64 `GraphMatcher.run()` returns)
    scores, status = result.scores.cpu().numpy(), result.status.cpu().numpy()
    write_csv(Path(args.out), names, scores, status)
    if args.actives:
        write_enrichment(Path(args.enrichment_out), result, labels, enrichment_cut, args.bedroc_alpha, args.bootstrap, args.bootstrap_seed)
    if args.similar_to:
        write_similar_csv(Path(args.similar_out), names, lib, queries, args.similar_to, args.similar_k)
    if args.explain > 0:
        # (a directory's hits are read again; a packed library's atoms come from its store)
        hits = Hits(names, scores, status, model, lib, weight, args.explain, store=store if packed else None, pocket=args.pocket, clash_level=args.clash_level,
                    tolerance=args.clash_tolerance, restraint=args.refine_restraint, max_iter=args.refine_iter)
        write_explain_csv(Path(args.explain_out) if args.explain_out else Path(str(args.out) + ".explain.csv"), hits)
        if args.modes is not None and not args.modes_out:
            args.modes_out = str(args.out) + ".modes.csv"
        for flag, path, writer, further in SIDE_REPORTS:
            if _asked(args, flag):
                writer(Path(getattr(args, path)), hits, *further(args))
    if args.diverse is not None:
        write_diverse_csv(Path(args.diverse_out), names, result, args.diverse, args.diverse_pool, args.diverse_threshold)
    if args.constrained_out:
        write_constrained_csv(Path(args.constrained_out), names, model, lib, weight, args.constrained_k, require, exclude)
    if args.panel_out or args.save_top:
        from .engine import DeviceLibrary

        dlib = lib if isinstance(lib, DeviceLibrary) else DeviceLibrary(lib)  # (resident once for both)
        if args.panel_out:
            write_panel_csv(Path(args.panel_out), names, scores, status, model, args.panel, dlib, weight, args.panel_k)
        if args.save_top:
            save_top(Path(args.save_top[1]), names, scores, status, dlib, save_k, store)  # (a packed library's store, where it has one, goes along too)


def write_enrichment(out: Path, result, labels: np.ndarray, cutoffs: list[float], alpha: float, bootstrap: int, seed: int) -> None:
    """`metric,value,ci_low,ci_high` of the screen against the labels (`engine.enrichment` on the float32 rounding of the screen's scores,
    which is what `pmx_score` returns): the numbers of actives and decoys, AUROC, BEDROC and the enrichment factor at every cutoff, with
    95 % percentile intervals over `bootstrap` resamples (empty without)."""
    import torch

    from .engine import enrichment
    from .validation import write_enrichment_csv

    en = enrichment(result.scores.to(torch.float32), labels, status=result.status, cutoffs=cutoffs, alpha=alpha, bootstrap=bootstrap, seed=seed)
    write_enrichment_csv(out, en)


def write_similar_csv(out: Path, names: list[str], lib, queries: list[int], query_names: list[str], k: int) -> None:
    """The k ligands of the library most similar to the query ligands by their own pharmacophore fingerprints (`engine.similar`: Tanimoto
    similarity of the two-point fingerprints over all conformers), best first, ties in library order: the maximum over the queries and
    one column per query, named by the query's file stem. The queries themselves are listed (each is 1.0 similar to itself)."""
    from .engine import similar

    res = similar(lib, query_indices=queries, k=min(k, len(names)))
    order, fused, per_query = res.topk_indices.cpu().numpy(), res.topk_scores.cpu().numpy(), res.scores.cpu().numpy()
    with open(out, "w") as w:
        w.write("rank,path,similarity," + ",".join(Path(q).stem for q in query_names) + "\n")
        for r, i in enumerate(order):
            w.write(f"{r + 1},{names[int(i)]},{float(fused[r])}," + ",".join(str(float(v)) for v in per_query[:, int(i)]) + "\n")


def write_panel_csv(out: Path, names: list[str], scores: np.ndarray, status: np.ndarray, model, panel: list[str], lib, weights, k: int) -> None:
    """The k best hits of a screen, in the order of the main CSV, against a panel of other pockets (`engine.screen_multi` on those k ligands
    only, gathered on the device): the hit's score, its float64 score against every panel model (a column named by the model file's stem) and
    the margin - the score minus the best panel score: what the hit has over its best off-target."""
    from .engine import screen_multi

    order = _best_hits(scores, status, k)
    res = screen_multi([model] + [PharmacophoreModel.load(m) for m in panel], lib, weights=weights, indices=order, float64=True)
    sc, margin = res.scores.cpu().numpy(), res.margin(0).cpu().numpy()
    with open(out, "w") as w:
        w.write("rank,path,score," + ",".join(Path(m).stem for m in panel) + ",margin\n")
        for r, i in enumerate(order):
            w.write(f"{r + 1},{names[i]},{float(sc[0, r])}," + ",".join(str(float(v)) for v in sc[1:, r]) + f",{float(margin[r])}\n")


def save_top(path: Path, names: list[str], scores: np.ndarray, status: np.ndarray, lib, k: int, store: PackedAtoms | None = None) -> None:
    """The k best hits of a screen, in the order of the main CSV, as a packed library file of their own (`DeviceLibrary.select`, read back with
    `download`) and its `.names` file: what `--library_dir` takes for the next campaign. With `store`, the library's atom store, the hits'
    heavy atoms go with them as `PATH.atoms` (`PackedAtoms.select`), so that the saved library can still be checked at atom level."""
    order = _best_hits(scores, status, k)
    sub = lib.select(order)
    sub.download().save(path)
    sub.close()
    Path(str(path) + ".names").write_text("".join(f"{names[i]}\n" for i in order))
    if store is not None:
        store.select(order).save(atoms_path(path))


def write_constrained_csv(out: Path, names: list[str], model, lib, weights, k: int, require, exclude) -> None:
    """The k best ligands by constrained score (`engine.screen_constrained`: only matches that hold a cluster of every `require` group
    and none of `exclude` count), best first: the constrained score, the ordinary score, the best conformer under the constraint and its
    matched pairs in the format of the explain CSV."""
    from .engine import screen_constrained

    res = screen_constrained(model, lib, k, require=require, exclude=exclude, weights=weights)
    if not res.exact:
        print("warning: the constrained hits are not certified exact (the pool of examined ligands was capped)", file=sys.stderr)
    ex = res.explanation
    types = model.flat.cluster_type
    with open(out, "w") as w:
        w.write("rank,path,constrained_score,score,best_conformer,matches\n")
        for r, i in enumerate(res.indices):
            c = int(ex.best_conformer[r])
            w.write(f"{r + 1},{names[int(i)]},{float(res.scores[r])},{float(res.unconstrained[r])},{c},{_matches(ex.levels[r], ex.match[r][c], types) if c >= 0 else ''}\n")


def write_diverse_csv(out: Path, names: list[str], result, k: int, pool: int | None, threshold: float) -> None:
    """The k first hits of the screen that are not the same binding mode again (`ScreeningResult.diverse`), best first: the hit's rank
    in the main CSV, its score, how many hits of the pool joined it (itself included) and the model nodes it engages."""
    dv = result.diverse(k, pool=pool, threshold=threshold)
    pool_rows = dv.profile.rows
    scores = result.scores.cpu().numpy()  # (the main CSV's numbers)
    with open(out, "w") as w:
        w.write("rank,path,score,cluster_size,engaged_nodes\n")
        for r, row in enumerate(dv.leaders):
            w.write(f"{int(pool_rows[row]) + 1},{names[int(dv.indices[r])]},{float(scores[int(dv.indices[r])])},{int(dv.cluster_size[r])},{' '.join(str(int(m)) for m in dv.profile.nodes(int(row)))}\n")


if __name__ == "__main__":
    main()

