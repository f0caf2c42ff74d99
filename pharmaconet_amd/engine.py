"""Host orchestration of the HIP engine: device handles, batched scoring, top-k.

PyTorch is used for what it is good at here - device buffers, the current HIP stream and (in
`distributed.py`) the RCCL process group; the arithmetic is all in libpmx.so.
"""

from __future__ import annotations

import contextlib
import ctypes
import dataclasses
from dataclasses import dataclass

import numpy as np

from . import _ffi
from ._device import (_FP_WORDS, _MAX_LEADERS, _MAX_LEVELS, _MAX_MODEL_NODES, _MAX_NODES, _MAX_QUERIES, NO_LEVEL, NO_MATCH, DeviceAtoms, DeviceLibrary,  # noqa: F401
                      _device_index, _is_store, _listed_indices, _ModelHandle, _record_counts, _resident, _resident_atoms, _torch,
                      _weights_array, device_model)
from .atoms import PackedAtoms  # noqa: F401
from .constants import weights_vector  # noqa: F401
from .library import PackedLibrary, as_packed_library  # noqa: F401
# the posed-hit layer (poses.py); every name of it stays importable from here
from .poses import (Alignment, ClashReport, ColourReport, ComboOverlay, PoseFit, RefinedPoses, ShapeOverlay, ShapeReport, ShapeStarts, _atomic_numbers, _fingerprint_tensor,  # noqa: F401
                    _heavy_atoms, _PocketHandle, _pose_source, _PoseRows, _ragged, _ratio, _ShapeRefHandle, clashes, device_pocket,
                    balanced_colour_weight, colour, colour_of, combo_overlay, combo_overlay_of, device_colour_ref, device_shape_ref, fingerprint_leaders, fingerprint_similarity, overlay, overlay_starts, pose_fit, refine, shape)
from .validation import ENRICH_TILE, FLOAT64_REFUSED, MAX_BOOTSTRAP, MAX_COLUMNS, POISSON1_CDF64, Enrichment, cutoffs_ppm  # noqa: F401  (the table and the tile of include/pmx.h)

__all__ = ["Alignment", "Attribution", "ClashReport", "DeviceAtoms", "DeviceLibrary", "FittingHits", "Enrichment", "Explanation", "LigandFingerprints", "PanelResult", "PoseFit", "ScreeningResult", "SimilarityResult", "align", "attribute", "clashes",
           "enrichment", "explain", "score_one", "screen", "screen_multi", "similar", "sweep", "topk", "device_model", "last_score_stats", "pose_fit", "ShapeReport", "shape",
           "device_shape_ref", "ColourReport", "ComboOverlay", "colour", "colour_of", "combo_overlay", "combo_overlay_of", "device_colour_ref"]


FEATURE_FIELDS = ("atom_off", "atomic_num", "nbr_off", "nbr", "feat_off", "feat_type", "feat_flags", "feat_atom_off", "feat_atoms",
                  "feat_center_off", "feat_centers", "n_conf", "pos_off", "positions")


def features_to_device(flat, device=None, non_blocking: bool = False) -> dict:
    """The arrays of `library.flatten_features` as device tensors (uint64 offsets travel as int64 bits)."""
    torch = _torch()
    dev = torch.device("cuda", _device_index(device))
    out = {}
    for k in FEATURE_FIELDS:
        a = flat[k]
        if not isinstance(a, torch.Tensor):
            a = np.ascontiguousarray(a)
            a = torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a)
        out[k] = a.to(dev, non_blocking=non_blocking)
    return out


def pack_bound(flat) -> int:
    """Upper bound of the packed size of a feature batch (every feature a node), as `pmx_pack_features`' sizing call computes it."""
    torch = _torch()
    feat_off, n_conf = flat["feat_off"], flat["n_conf"]
    if isinstance(feat_off, torch.Tensor):
        nf = (feat_off[1:] - feat_off[:-1]).to(torch.int64)
        c = n_conf.to(torch.int64).clamp(min=1)
        return int(((((8 + 2 * nf + 3 + 12 * nf * c + 15) // 16) * 16) + 16).sum().item())
    nf = np.diff(np.asarray(feat_off).astype(np.int64))
    c = np.maximum(np.asarray(n_conf).astype(np.int64), 1)
    return int((((8 + 2 * nf + 3 + 12 * nf * c + 15) & ~15) + 16).sum())


def pack_features_device(flat, device=None, out=None, bound: int | None = None):
    """`pmx_pack_features_device` (csrc/pmx_pack_device.hip): LigandGraph + priority sort on the device, on torch's current stream.
    Returns (offsets int64 [n + 1], data uint8 [bytes], status int32 [n]) as device tensors; records byte-identical to
    `library.pack_features_native`. `out` = (offsets, data, status) tensors to write into (data at least `pack_bound(flat)` long)."""
    torch = _torch()
    lib = _ffi.load()
    dev_index = _device_index(device if device is not None else (flat["positions"].device if isinstance(flat["positions"], torch.Tensor) else None))
    tdev = torch.device("cuda", dev_index)
    if not all(isinstance(flat[k], torch.Tensor) and flat[k].is_cuda for k in FEATURE_FIELDS):
        flat = features_to_device(flat, tdev)
    n = int(flat["atom_off"].numel()) - 1
    if out is None:
        cap = int(bound) if bound is not None else pack_bound(flat)
        out = (torch.empty(n + 1, dtype=torch.int64, device=tdev), torch.empty(max(cap, 16), dtype=torch.uint8, device=tdev),
               torch.empty(max(n, 1), dtype=torch.int32, device=tdev))
    offsets, data, status = out
    batch = _ffi.FeatureBatch(n, *(flat[k].data_ptr() for k in FEATURE_FIELDS))
    nbytes = ctypes.c_uint64(0)
    with torch.cuda.device(tdev):
        stream = torch.cuda.current_stream(tdev).cuda_stream
        _ffi.check(lib.pmx_pack_features_device(ctypes.byref(batch), dev_index, ctypes.c_void_p(stream), offsets.data_ptr(), data.data_ptr(), int(data.numel()),
                                                ctypes.byref(nbytes), status.data_ptr()))
    return offsets[: n + 1], data[: int(nbytes.value)], status[:n]


@dataclass
class ScreeningResult:
    scores: "object"  # torch.float32 (float64 with `screen(..., float64=True)`) [count] on the device, library order
    status: "object"  # torch.int32 [count]
    first: int
    topk_scores: "object | None" = None  # torch.float32 [k]
    topk_indices: "object | None" = None  # torch.int64 [k], global ligand indices (first + position)
    model: "object | None" = None  # what `screen` scored (for `explain`): the model, the library when it was a DeviceLibrary or a PackedLibrary
    library: "object | None" = None
    weights: "dict | None" = None
    index_base: int = 0  # added to library indices in topk_indices
    indices: "object | None" = None  # a listed screen (`screen(..., indices=)`): torch.int64 [count] on the device, the library ligand behind each score

    def scores_numpy(self) -> np.ndarray:
        return self.scores.cpu().numpy()

    def ranking(self) -> list[tuple[int, float]]:
        """[(ligand index, score)] of the top-k, best first (the order of screening.py:70-75)."""
        assert self.topk_scores is not None and self.topk_indices is not None
        idx = self.topk_indices.cpu().numpy()
        sc = self.topk_scores.cpu().numpy()
        return [(int(i), float(s)) for i, s in zip(idx, sc) if i >= 0]

    def explain(self, k: int, model=None, library=None, weights: dict[str, float] | None = None) -> "Explanation":
        """`explain` of this screen's k best ligands (best first), without scoring the library again. `model`, `library` and `weights`
        default to what `screen` was called with."""
        model, library, weights = self._scored(model, library, weights)
        return explain(model, library, self._best(k), weights=weights)

    def _scored(self, model, library, weights):
        model = model if model is not None else self.model
        library = library if library is not None else self.library
        weights = self.weights if weights is None else weights
        if model is None or library is None:
            raise ValueError("this result does not know its library (it was not given as a DeviceLibrary or a PackedLibrary): pass it")
        return model, library, weights

    def _best(self, k: int) -> np.ndarray:
        """Library indices of this screen's k best ligands, best first."""
        if self.topk_indices is not None and int(self.topk_indices.numel()) >= k:
            top = self.topk_indices.cpu().numpy()[:k]
            idx = top[top >= 0] - self.index_base  # (global indices of a sharded screen -> library indices)
        else:
            sc = self.scores.cpu().numpy().astype(np.float64)
            key = np.where(self.status.cpu().numpy() != 0, -np.inf, np.nan_to_num(sc, nan=-np.inf))
            idx = np.lexsort((np.arange(len(sc)), -key))[:k] + self.first
            if self.indices is not None:  # (a listed screen: positions of the list -> library indices)
                idx = self.indices.cpu().numpy()[idx]
        return np.asarray([i for i in idx if i >= 0], dtype=np.uint64)

    def panel(self, k: int, models, library=None) -> "PanelResult":
        """This screen's k best ligands (best first) against other pockets: a `PanelResult` whose column 0 is this screen's own model and whose
        further columns are `models`, under this screen's weights and in its precision - `DeviceLibrary.select` of the hits, then `screen_multi`."""
        model, library, weights = self._scored(None, library, None)
        return screen_multi([model, *models], library, weights=weights, indices=self._best(k).astype(np.int64), float64=str(self.scores.dtype).endswith("float64"))

    def enrichment(self, labels, **kwargs) -> "Enrichment":
        """`enrichment` of this screen's scores and status: does the model rank the actives of `labels` above its decoys? `labels` are in the
        order of the scores (list order for a listed screen)."""
        return enrichment(self.scores, labels, status=self.status, **kwargs)

    def modes(self, k: int, modes: int = 4, model=None, library=None, weights: dict[str, float] | None = None, require=None, exclude=None) -> "ModeSet":
        """`explain_modes` of this screen's k best ligands (the rows of `explain(k)`): the `modes` best binding modes per conformer."""
        model, library, weights = self._scored(model, library, weights)
        return explain_modes(model, library, self._best(k), modes=modes, weights=weights, require=require, exclude=exclude)

    def overlay(self, k: int, reference, atoms=None, starts: int = 4, conformers: str = "best", model=None, library=None, weights: dict[str, float] | None = None,
                **kw) -> "ShapeOverlay":
        """`overlay` of this screen's k best ligands (best first) on a known ligand: ligand-based shape screening of a screen's top hits.
        The points are the hits' pharmacophore nodes, or their heavy atoms with `atoms` (the library's atom store).
          conformers="best"   each hit at the conformer of its best match (`explain(k).poses`); with `starts=0` from that fitted pose,
                              with `starts=4` from the four inertial starts
          conformers="all"    every conformer of each hit from the inertial starts (`starts=4`), keeping per hit the conformer of highest
                              final Tanimoto, the lower among equals
        k * conformers * starts may not exceed 65536 rows. Further arguments (`node_radius`, `ftol`, `max_iter`) as `overlay` takes them."""
        model, library, weights = self._scored(model, library, weights)
        source = (lambda idx, conf: dict(atoms=atoms, indices=idx, conformers=conf)) if atoms is not None else (lambda idx, conf: dict(library=library, indices=idx, conformers=conf))
        return self._overlay_hits("overlay", "tanimoto", k, starts, conformers, model, library, weights,
                                  lambda al: al.overlay(reference, library if atoms is None else None, atoms=atoms, **kw),
                                  lambda idx, conf: overlay(reference, starts=starts, **source(idx, conf), **kw))

    def _overlay_hits(self, name, field, k, starts, conformers, model, library, weights, from_poses, from_starts):
        """What `overlay` and `combo_overlay` do with this screen's k best ligands: `from_poses(alignment)` runs the call from the fitted
        poses (`starts=0`), `from_starts(indices, conformers)` from the inertial starts; with `conformers="all"` the conformer of highest
        final `field` is kept per hit, the lower among equals. `name` names the method in a message."""
        what = f"ScreeningResult.{name}"
        if conformers not in ("best", "all"):
            raise ValueError(f"{what}: conformers is 'best' or 'all'")
        if starts not in (0, 4):
            raise ValueError(f"{what}: starts is 0 or 4")
        if conformers == "best":
            if k * max(starts, 1) > _ffi.EXPLAIN_MAX:
                raise ValueError(f"{what}: {k} hits x {max(starts, 1)} starts exceed {_ffi.EXPLAIN_MAX} rows")
            al = explain(model, library, self._best(k), weights=weights).poses(model, library, weights=weights)
            return from_poses(al) if starts == 0 else from_starts(al.indices, al.conformers)
        if starts == 0:
            raise ValueError(f"{what}: conformers='all' has a fitted pose for one conformer only; use starts=4")
        hits = self._best(k).astype(np.int64)
        with _resident(library) as dlib:
            n_conf = np.maximum(_record_counts(dlib, hits, 1), 1)
        rows = int(n_conf.sum()) * starts
        if rows > _ffi.EXPLAIN_MAX:
            raise ValueError(f"{what}: {len(hits)} hits x their conformers x {starts} starts are {rows} rows, more than {_ffi.EXPLAIN_MAX}; lower k or use conformers='best'")
        idx, conf = np.repeat(hits, n_conf), np.concatenate([np.arange(c) for c in n_conf]) if len(hits) else np.zeros(0, np.int64)
        every = from_starts(idx, conf)
        first = np.concatenate([[0], np.cumsum(n_conf)[:-1]]).astype(np.int64) if len(hits) else np.zeros(0, np.int64)
        value = np.where(np.isnan(getattr(every, field)), -np.inf, getattr(every, field))
        pick = np.array([lo + int(np.argmax(value[lo: lo + c])) for lo, c in zip(first, n_conf)], dtype=np.int64)  # (the first among equals)
        take = lambda v: v[pick] if isinstance(v, np.ndarray) else v  # noqa: E731  (None, or the one number colour_weight)
        return type(every)(**{f.name: take(getattr(every, f.name)) for f in dataclasses.fields(every)})

    def combo_overlay(self, k: int, reference, atoms=None, starts: int = 4, conformers: str = "best", model=None, library=None, weights: dict[str, float] | None = None,
                      **kw) -> "ComboOverlay":
        """`combo_overlay` of this screen's k best ligands (best first) on a known ligand that carries its typed features
        (`ReferenceLigand.from_library`, or `colour=` a `shape.ColourFeatures`): shape plus colour, the "TanimotoCombo" of ligand-based
        screening, of a screen's top hits. The typed points are the hits' pharmacophore nodes; the shape points are those nodes, or the
        heavy atoms with `atoms` (the library's atom store). `conformers` and `starts` as `overlay` has them, `conformers="all"` keeping
        per hit the conformer of highest final combo, the lower among equals. Further arguments (`colour_weight`, `node_radius`, `ftol`,
        `max_iter`) as `combo_overlay` takes them."""
        model, library, weights = self._scored(model, library, weights)
        if atoms is not None and not _is_store(atoms):
            raise TypeError("ScreeningResult.combo_overlay: atoms is the library's DeviceAtoms / PackedAtoms")
        return self._overlay_hits("combo_overlay", "combo", k, starts, conformers, model, library, weights,
                                  lambda al: combo_overlay_of(al, reference, library, atoms=atoms, **kw),
                                  lambda idx, conf: combo_overlay(reference, library, idx, conf, atoms=atoms, starts=starts, **kw))

    def diverse(self, k: int, pool: int | None = None, threshold: float = 0.7, model=None, library=None, weights: dict[str, float] | None = None) -> "DiverseHits":
        """The k first hits of this screen that are not the same binding mode again: the best `pool` hits (default
        min(len, max(8 k, 1024), 65536)) are explained, fingerprinted at their best conformer (`Explanation.hotspots`) and run through
        `HotspotProfile.leaders(threshold)` in rank order. Hits with a non-zero status are left out of the pool."""
        if k <= 0:
            raise ValueError("k must be positive")
        model, library, weights = self._scored(model, library, weights)
        n = int(self.scores.numel())
        pool = min(n, max(8 * k, 1024), 65536) if pool is None else int(pool)
        if not 0 < pool <= 65536:
            raise ValueError("pool: 1 to 65536 hits")
        ex = explain(model, library, self._best(pool), weights=weights)
        prof = ex.hotspots(model, library, weights=weights)
        leaders, leader_of = prof.leaders(threshold=threshold, max_leaders=min(k, 2048))
        sizes = np.bincount(leader_of[leader_of >= 0], minlength=len(prof)).astype(np.int64)
        return DiverseHits(indices=prof.indices[leaders], scores=ex.scores[prof.rows[leaders]], cluster_size=sizes[leaders],
                           leaders=leaders, leader_of=leader_of, pool=prof.indices, profile=prof)

    def diverse_ligands(self, k: int, pool: int | None = None, threshold: float = 0.7, library=None) -> "DiverseHits":
        """The k first hits of this screen that are not the same ligand again: `diverse` with the ligand's own fingerprint in place of the
        binding mode's. The best `pool` hits (`diverse`'s rule: default min(len, max(8 k, 1024), 65536), hits with a non-zero status
        left out) are gathered (`DeviceLibrary.select`), fingerprinted over all their conformers (`DeviceLibrary.fingerprints`) and run
        through `LigandFingerprints.leaders(threshold)` in rank order. Two analogues in two binding modes are one cluster here and two
        for `diverse`; two scaffolds in one mode the other way round. `profile` of the result is None."""
        if k <= 0:
            raise ValueError("k must be positive")
        _, library, _ = self._scored(self.model, library, None)
        n = int(self.scores.numel())
        pool = min(n, max(8 * k, 1024), 65536) if pool is None else int(pool)
        if not 0 < pool <= 65536:
            raise ValueError("pool: 1 to 65536 hits")
        sc, st = self.scores.cpu().numpy().astype(np.float64), self.status.cpu().numpy()
        key = np.where(st != 0, -np.inf, np.nan_to_num(sc, nan=-np.inf))
        pos = np.lexsort((np.arange(n), -key))[:pool]  # (the order of `_best`)
        pos = pos[st[pos] == 0]
        idx = (self.indices.cpu().numpy()[pos] if self.indices is not None else pos + self.first).astype(np.int64)
        with _resident(library) as dlib:
            sub = dlib.select(idx)
            try:
                leaders, leader_of = sub.fingerprints().leaders(threshold=threshold, max_leaders=min(k, 2048))
            finally:
                sub.close()
        sizes = np.bincount(leader_of[leader_of >= 0], minlength=len(idx)).astype(np.int64)
        return DiverseHits(indices=idx[leaders].astype(np.uint64), scores=sc[pos][leaders], cluster_size=sizes[leaders], leaders=leaders, leader_of=leader_of,
                           pool=idx.astype(np.uint64), profile=None)

    def fitting(self, k: int, pool: int | None = None, max_clashing: int = 0, pocket=None, atoms=None, model=None, library=None,
                weights: dict[str, float] | None = None, refine: bool = False, search: int = 0, fit: bool = False, shape=None, colour=None, **kw) -> "FittingHits":
        """The k first hits of this screen whose pose fits the pocket: the best `pool` hits (default min(len, max(8 k, 1024), 65536)) are
        explained, posed at their best conformer (`Explanation.poses`) and checked against the protein's atoms (`Alignment.clashes`); a hit
        passes with status 0 and at most `max_clashing` clashing points. In rank order; a hit that was not scored, or whose pose is not OK,
        never passes. `pocket`: a `pocket.PocketAtoms` (default: the protein the model carries). `atoms`: a function from a library index to
        the `LigandFeatures` / `Ligand` of that ligand, for a check of the molecule's atoms; without it the pharmacophore nodes are checked.
        Further arguments (`tolerance`, `contact`, `node_radius`) as `clashes` takes them.
        With `refine`, a pose that fails the check is moved out of the protein's atoms (`Alignment.refine`) and checked again; `poses` and
        `report` then describe the poses as used - the refined one where the fitted one failed - and `refined` has the refinement of every
        posed hit: one call refines all rows of the pool (a row keeps its place, and the call costs milliseconds), but only
        the motions of the rows that failed are used. The fit fields of `poses` (`rmsd`, `sse`, `node`, ...) still describe the
        least-squares fit, not the refined motion; `refined.anchor_rmsd` says how far that moved. `restraint`, `max_iter` and `ftol` go to `refine`, and `refine_tolerance` is the tolerance it runs at (default: the
        check's; a penalty balanced against a restraint leaves a little overlap, so a smaller one is what makes grazing poses pass).
        With `search` = M > 0, a hit is posed not at its best conformer alone but where `pose_search` over all its conformers and their M
        best binding modes puts it: the best-scoring pose whose nodes pass, else the one of smallest overlap - which is then what `refine`
        starts from. `min_fraction` and `min_fitted` go to the search (a pose worth less than `min_fraction` of the hit's best is not
        considered). `poses` has a row for every hit that was scored; one without any pose has conformer -1 and never passes. `atoms`
        as a function verifies the chosen poses exactly as without the search.
        `atoms` may also be the library's atom store (a `DeviceAtoms` / `PackedAtoms`): the molecules' atoms are then taken from it on the
        device, and with `search` the search itself chooses on the atoms (`pose_search(atoms=...)`), so that what it picks is what the
        check accepts.
        With `fit`, `FittingHits.fit` is the `PoseFit` of every posed hit (`Alignment.pose_fit`, free mode) at the motion finally used -
        the refined one where the refinement was used; nothing else changes.
        With `shape` - a `shape.ReferenceLigand`, the known binder - `FittingHits.shape` is the `ShapeReport` of every posed hit
        (`Alignment.shape`) at the motion finally used, on the points the clash check read (the molecules' atoms with `atoms`, the nodes
        otherwise; `shape_cover` is its `cover`); nothing else changes.
        With `colour` - a `shape.ColourFeatures`, or a `ReferenceLigand` that carries one - `FittingHits.colour` is the `ColourReport` of
        every posed hit's nodes (`colour_of`) at the motion finally used (`colour_cover` is its `cover`); nothing else changes."""
        colour_kw = {"cover": kw.pop("colour_cover")} if "colour_cover" in kw else {}
        if colour_kw and colour is None:
            raise ValueError("colour_cover: an argument of the colour report, which is off (colour=reference)")
        shape_kw = {"cover": kw.pop("shape_cover")} if "shape_cover" in kw else {}
        if shape_kw and shape is None:
            raise ValueError("shape_cover: an argument of the shape report, which is off (shape=reference)")
        if k <= 0:
            raise ValueError("k must be positive")
        search = int(search)
        if not 0 <= search <= _ffi.MAX_MODES:
            raise ValueError(f"search: 0 (off) or 1 to {_ffi.MAX_MODES} binding modes")
        search_kw = {name: kw.pop(name) for name in ("min_fraction", "min_fitted") if name in kw}
        if search_kw and not search:
            raise ValueError(f"{sorted(search_kw)}: arguments of the pose search, which is off (search=M)")
        refine_kw = {name: kw.pop(name) for name in ("restraint", "max_iter", "ftol", "refine_tolerance") if name in kw}
        if refine_kw and not refine:
            raise ValueError(f"{sorted(refine_kw)}: arguments of the refinement, which is off (refine=True)")
        model, library, weights = self._scored(model, library, weights)
        n = int(self.scores.numel())
        pool = min(n, max(8 * k, 1024), 65536) if pool is None else int(pool)
        if not 0 < pool <= 65536:
            raise ValueError("pool: 1 to 65536 hits")
        pocket = model.pocket_atoms() if pocket is None else pocket
        with contextlib.ExitStack() as stack:
            dlib = stack.enter_context(_resident(library))
            store = stack.enter_context(_resident_atoms(atoms, dlib.device)) if _is_store(atoms) else None  # (uploaded once for all the calls below)
            if search:
                shared = {name: kw[name] for name in ("tolerance", "contact", "node_radius") if name in kw}
                ms = explain_modes(model, dlib, self._best(pool), modes=search, weights=weights)
                ps = ms.pose_search(model, dlib, pocket, weights=weights, max_clashing=max_clashing, atoms=store, **shared, **search_kw)
                ex = ms.explanation(0)  # (the hits' scores, as without the search)
                scored = np.flatnonzero(ps.status == 0)
                al = ps.alignment()
                al = dataclasses.replace(al, **{f.name: ([getattr(al, f.name)[r] for r in scored] if isinstance(getattr(al, f.name), list) else getattr(al, f.name)[scored])
                                                for f in dataclasses.fields(al)})  # (`rows`, the hit behind each row, becomes `scored`)
            else:
                ex = explain(model, dlib, self._best(pool), weights=weights)
                al = ex.poses(model, dlib, weights=weights)
            mols = None if atoms is None else store if store is not None else [atoms(int(i)) for i in al.indices]
            rep = al.clashes(pocket, dlib, atoms=mols, **kw)
            refined = None
            failing = ~rep.ok(max_clashing) & (al.status == 0)
            if refine and failing.any():
                shared = {name: kw[name] for name in ("tolerance", "node_radius", "device") if name in kw}
                if "refine_tolerance" in refine_kw:
                    shared["tolerance"] = refine_kw.pop("refine_tolerance")
                refined = al.refine(pocket, dlib, atoms=mols, **shared, **refine_kw)
                use = failing & (refined.status == 0)
                al = dataclasses.replace(al, rotation=np.where(use[:, None, None], refined.rotation, al.rotation),
                                         translation=np.where(use[:, None], refined.translation, al.translation))
                rep = al.clashes(pocket, dlib, atoms=mols, **kw)  # (a row that was not refined has the bits it had)
            pf = al.pose_fit(model, dlib, weights=weights) if fit else None
            sh = None
            if shape is not None:
                if "node_radius" in kw:
                    shape_kw["node_radius"] = kw["node_radius"]
                if "device" in kw:
                    shape_kw["device"] = kw["device"]
                sh = al.shape(shape, dlib, atoms=mols, **shape_kw)
            col = colour_of(al, colour, dlib, **colour_kw) if colour is not None else None
        passing = np.flatnonzero(rep.ok(max_clashing) & (al.status == 0))[:k]
        return FittingHits(indices=al.indices[passing].astype(np.uint64), scores=ex.scores[al.rows[passing]], ranks=al.rows[passing].astype(np.int64), rows=passing,
                           pool=ex.indices, poses=al, report=rep, refined=refined, fit=pf, shape=sh, colour=col)

    def similar_to(self, rank: int, k: int = 100, library=None) -> "SimilarityResult":
        """The library's neighbours of this screen's hit at `rank` (0 is the best hit): `similar` with that ligand as the one query,
        fingerprinted at the conformer that explains its score (`Explanation.best_conformer`) - the hit as it is posed - against the union
        fingerprints of the library."""
        model, library, weights = self._scored(None, library, None)
        best = self._best(int(rank) + 1)
        if rank < 0 or len(best) <= rank:
            raise IndexError(f"this screen has no hit at rank {rank}")
        hit = int(best[rank])
        with _resident(library) as dlib:
            ex = explain(model, dlib, [hit], weights=weights)
            if int(ex.status[0]) != 0:
                raise ValueError(f"the hit at rank {rank} was not scored (status {int(ex.status[0])})")
            return similar(dlib, query_indices=[hit], query_conformers=[int(ex.best_conformer[0])], k=k)


def topk(scores, k: int, base_index: int = 0, indices=None):
    """k best of a device float32 tensor: (scores [k], int64 global indices [k]); ties by ascending index.

    The library is handed addresses and a count, so what it would read as other bytes is refused here (ValueError): `scores` must be a
    contiguous float32 tensor on a GPU, `indices` (if given) a contiguous int64 tensor of the same length on the same device, k >= 0."""
    import torch

    k = int(k)
    if scores.dtype != torch.float32 or not scores.is_contiguous():
        raise ValueError(f"topk: scores must be a contiguous float32 tensor, not {scores.dtype}{'' if scores.is_contiguous() else ' (not contiguous)'}")
    if k < 0:
        raise ValueError(f"topk: k must not be negative, not {k}")
    if indices is not None:
        if indices.dtype != torch.int64 or not indices.is_contiguous():
            raise ValueError(f"topk: indices must be a contiguous int64 tensor, not {indices.dtype}{'' if indices.is_contiguous() else ' (not contiguous)'}")
        if indices.numel() != scores.numel():
            raise ValueError(f"topk: {indices.numel()} indices for {scores.numel()} scores")
        if indices.device != scores.device:
            raise ValueError(f"topk: indices on {indices.device}, scores on {scores.device}")
    if not scores.is_cuda:
        raise ValueError(f"topk: scores must be on a GPU, not on {scores.device}")
    torch = _torch()
    lib = _ffi.load()
    dev = scores.device.index
    out_s = torch.empty(k, dtype=torch.float32, device=scores.device)
    out_i = torch.empty(k, dtype=torch.int64, device=scores.device)
    stream = torch.cuda.current_stream(scores.device).cuda_stream
    _ffi.check(
        lib.pmx_topk(
            scores.data_ptr(),
            indices.data_ptr() if indices is not None else None,
            scores.numel(),
            base_index,
            k,
            out_s.data_ptr(),
            out_i.data_ptr(),
            dev,
            ctypes.c_void_p(stream),
        )
    )
    return out_s, out_i


def screen(
    model,
    library,
    weights: dict[str, float] | None = None,
    topk: int | None = None,
    device=None,
    first: int = 0,
    count: int | None = None,
    index_base: int = 0,
    float64: bool = False,
    indices=None,
) -> ScreeningResult:
    """Score ligands `[first, first + count)` of `library` against `model` on the GPU.

    `library` is a `DeviceLibrary` (already in HBM) or anything `as_packed_library` accepts.
    `index_base` is added to positions when reporting top-k indices (the shard's global offset).
    `indices` (instead of `first` / `count`): a listed screen - the ligands `indices` (a list, a NumPy array or an int64 device tensor; any
    order, repeats allowed), gathered on the device (`DeviceLibrary.select`) and scored as a library of their own. Scores and status
    come back in list order, `topk_indices` are indices of `library` (ties in list order), and the result's `explain` / `modes` explain
    against `library`.
    `float64`: scores as the float64 the reference returns (`pmx_score_f64`; `graph_match.py:109`) instead of its float32
    rounding; the device top-k ranks float32 values, so it is not offered together with `topk`."""
    torch = _torch()
    lib = _ffi.load()
    if float64 and topk is not None:
        raise ValueError(FLOAT64_REFUSED)
    with _resident(library, device) as whole, _listed(whole, indices, first, count) as (dlib, listed, first, count):
        dev = dlib.device
        mh = device_model(model, dev)
        tdev = torch.device("cuda", dev)
        scores = torch.empty(count, dtype=torch.float64 if float64 else torch.float32, device=tdev)
        status = torch.empty(count, dtype=torch.int32, device=tdev)
        stream = torch.cuda.current_stream(tdev).cuda_stream
        _ffi.check(
            (lib.pmx_score_f64 if float64 else lib.pmx_score)(
                mh.handle, dlib.handle, _weights_array(weights), first, count,
                scores.data_ptr(), status.data_ptr(), ctypes.c_void_p(stream),
            )
        )
        result = ScreeningResult(scores=scores, status=status, first=first, model=model, library=library if isinstance(library, (DeviceLibrary, PackedLibrary)) else None,
                                  weights=weights, index_base=index_base, indices=listed)
        if topk is not None and listed is not None:  # (pmx_topk breaks ties by position: list order)
            result.topk_scores, result.topk_indices = globals()["topk"](scores, int(topk), indices=listed + index_base if index_base else listed)
        elif topk is not None:
            result.topk_scores, result.topk_indices = globals()["topk"](scores, int(topk), base_index=index_base + first)
    return result


@contextlib.contextmanager
def _listed(dlib: "DeviceLibrary", indices, first: int, count: int | None):
    """What a scoring call scores: (library, None, first, count) for the range `[first, first + count)` of `dlib`; for a list of ligands
    (`indices`) the selection as a library of its own with the list on the device and the range that covers it, closed behind the block. The
    selection's buffers are torch's, allocated on the stream the scoring call is enqueued on, so they may be given back while it still runs."""
    if indices is None:
        yield dlib, None, first, (len(dlib) - first if count is None else count)
        return
    if first != 0 or count is not None:
        raise ValueError("`indices` and `first` / `count` are mutually exclusive")
    torch = _torch()
    listed = _listed_indices(indices, torch.device("cuda", dlib.device))
    sub = dlib.select(listed)
    try:
        yield sub, listed, 0, len(sub)
    finally:
        sub.close()


@dataclass
class PanelResult:
    """What `screen_multi` returns: one library (or one list of its ligands) against several pockets.

    scores   torch.float32 (float64 with `float64=True`) [n_models, count] on the device: row m is what `screen(models[m], ...)` gives
    status   torch.int32 [count]: PMX_LIGAND_*, the same for every pocket
    indices  torch.int64 [count] on the device for a listed call (the library ligand behind each column), else None: column j is ligand first + j"""

    scores: "object"
    status: "object"
    first: int = 0
    indices: "object | None" = None
    models: "list | None" = None
    library: "object | None" = None
    weights: "dict | None" = None

    def ligands(self) -> np.ndarray:
        """int64 [count]: the library ligand behind each column."""
        return self.indices.cpu().numpy() if self.indices is not None else np.arange(int(self.status.numel()), dtype=np.int64) + self.first

    def best(self, m: int, k: int) -> tuple[np.ndarray, np.ndarray]:
        """(library indices, scores) of pocket m's k best ligands, best first; ties in column order, ligands with a non-zero status left out."""
        sc, st = self.scores[m].cpu().numpy(), self.status.cpu().numpy()
        key = np.where(st != 0, -np.inf, np.nan_to_num(sc.astype(np.float64), nan=-np.inf))
        cols = [int(j) for j in np.lexsort((np.arange(len(sc)), -key))[:k] if st[j] == 0]
        return self.ligands()[cols], sc[cols]

    def enrichment(self, labels, **kwargs) -> "Enrichment":
        """`enrichment` with one column per pocket of the panel (`labels` in the order of `ligands()`): `delta(a, b, metric)` of the result
        compares two pockets' models on the same resamples."""
        return enrichment(self.scores, labels, status=self.status, **kwargs)

    def margin(self, target: int):
        """[count] on the device: the target pocket's score minus the best score of the other pockets - how selective each ligand is for it."""
        n = int(self.scores.shape[0])
        if n < 2 or not 0 <= target < n:
            raise ValueError(f"margin of pocket {target} among {n}: needs a pocket of the panel and at least one other")
        others = [m for m in range(n) if m != target]
        return self.scores[target] - self.scores[others].max(dim=0).values


def screen_multi(models, library, weights: dict[str, float] | None = None, first: int = 0, count: int | None = None, indices=None, float64: bool = False,
                 device=None) -> PanelResult:
    """Score ligands `[first, first + count)` of `library`, or the ligands `indices`, against every model of `models` in one call
    (`pmx_score_multi` / `pmx_score_multi_f64`: one pocket after the other on torch's current stream, the library read from HBM each time).
    `library`, `indices` and `float64` as `screen` takes them; each row of the result's scores is bit for bit that pocket's `screen`."""
    torch = _torch()
    lib = _ffi.load()
    models = list(models)
    with _resident(library, device) as whole, _listed(whole, indices, first, count) as (dlib, listed, first, count):
        tdev = torch.device("cuda", dlib.device)
        handles = (ctypes.c_void_p * max(len(models), 1))(*(device_model(m, dlib.device).handle.value for m in models))
        scores = torch.empty((len(models), count), dtype=torch.float64 if float64 else torch.float32, device=tdev)
        status = torch.empty(count, dtype=torch.int32, device=tdev)
        stream = torch.cuda.current_stream(tdev).cuda_stream
        _ffi.check((lib.pmx_score_multi_f64 if float64 else lib.pmx_score_multi)(handles, len(models), dlib.handle, _weights_array(weights), first, count,
                                                                                   scores.data_ptr(), status.data_ptr(), ctypes.c_void_p(stream)))
    return PanelResult(scores=scores, status=status, first=first, indices=listed, models=models,
                       library=library if isinstance(library, (DeviceLibrary, PackedLibrary)) else None, weights=weights)


def _labels_tensor(labels, n: int, tdev):
    """Labels (bool / uint8: 0 decoy, 1 active, 2 not counted) as a uint8 tensor [n] on `tdev`; a host array is checked here, a device
    tensor by the call itself (`pmx_enrichment` marks its totals)."""
    torch = _torch()
    if isinstance(labels, torch.Tensor):
        if labels.dtype not in (torch.bool, torch.uint8):
            raise TypeError("labels as a tensor: bool or uint8")
        t = labels.to(tdev).to(torch.uint8).reshape(-1).contiguous()
    else:
        host = np.asarray(labels)
        if host.dtype != np.bool_ and host.dtype != np.uint8:
            if not np.issubdtype(host.dtype, np.integer):
                raise TypeError("labels: a bool or uint8 array")
        if host.size and (host.astype(np.int64).min() < 0 or host.astype(np.int64).max() > 2):
            raise ValueError("labels: 0 (decoy), 1 (active) or 2 (not counted)")
        t = torch.from_numpy(np.ascontiguousarray(host.astype(np.uint8).reshape(-1))).to(tdev)
    if int(t.numel()) != n:
        raise ValueError(f"{int(t.numel())} labels for {n} scores")
    return t


def enrichment(scores, labels, status=None, cutoffs=(0.005, 0.01, 0.05), alpha: float = 20.0, bootstrap: int = 0, seed: int = 0, order: bool = False,
               columns=None) -> Enrichment:
    """Retrospective validation of one or more columns of scores over a labelled list (`pmx_enrichment`, include/pmx.h): AUROC, the
    enrichment factor at each of `cutoffs` (fractions of the list) and BEDROC(`alpha`), each the expectation under random tie-breaking,
    for the sample and for `bootstrap` Poisson resamples of it (seeded; a ligand has the same count in every column).

    `scores`: float32 device tensor [n] or [n_cols, n] (`ScreeningResult.scores`, `PanelResult.scores`); `status`: int32 [n] or None;
    `labels`: bool / uint8 array or device tensor [n] - 0 decoy, 1 active, 2 not counted. `order=True` also returns the ranked ligand
    indices of every column. The call is enqueued on torch's current stream behind the producer of `scores`; the results are read back."""
    torch = _torch()
    lib = _ffi.load()
    if not isinstance(scores, torch.Tensor) or not scores.is_cuda:
        raise TypeError("scores: a float32 tensor on the device")
    if scores.dtype == torch.float64:
        raise ValueError(FLOAT64_REFUSED)
    if scores.dtype != torch.float32 or scores.dim() not in (1, 2):
        raise TypeError("scores: a float32 tensor [n] or [n_cols, n]")
    sc = scores if scores.dim() == 2 else scores.reshape(1, -1)
    if sc.stride(1) != 1 or (sc.shape[0] > 1 and sc.stride(0) < sc.shape[1]):
        sc = sc.contiguous()
    n_cols, n = int(sc.shape[0]), int(sc.shape[1])
    if n < 1 or not 1 <= n_cols <= MAX_COLUMNS:
        raise ValueError(f"enrichment: at least one ligand and 1 to {MAX_COLUMNS} columns")
    if not 0 <= int(bootstrap) <= MAX_BOOTSTRAP:
        raise ValueError(f"bootstrap: 0 to {MAX_BOOTSTRAP} resamples")
    if not alpha > 0:
        raise ValueError("alpha must be positive")
    tdev = sc.device
    ppm = cutoffs_ppm(cutoffs)
    lab = _labels_tensor(labels, n, tdev)
    st = None
    if status is not None:
        st = (status if isinstance(status, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(status, dtype=np.int32)))).to(tdev).to(torch.int32).reshape(-1).contiguous()
        if int(st.numel()) != n:
            raise ValueError(f"{int(st.numel())} status values for {n} scores")
    rows, n_cut = 1 + int(bootstrap), len(ppm)
    totals = torch.empty((rows, 3), dtype=torch.int64, device=tdev)
    u2 = torch.empty((n_cols, rows), dtype=torch.int64, device=tdev)
    hits = torch.empty((n_cols, rows, n_cut), dtype=torch.float64, device=tdev)
    expsum = torch.empty((n_cols, rows), dtype=torch.float64, device=tdev)
    ranked = None
    if order:
        n_counted = int((lab < 2).sum().item())
        ranked = torch.empty((n_cols, n_counted), dtype=torch.int64, device=tdev)
    stream = torch.cuda.current_stream(tdev).cuda_stream
    _ffi.check(lib.pmx_enrichment(sc.data_ptr(), int(sc.stride(0)) if n_cols > 1 else n, n_cols, n, st.data_ptr() if st is not None else None, lab.data_ptr(),
                                  (ctypes.c_uint32 * max(n_cut, 1))(*(int(p) for p in ppm)), n_cut, float(alpha), int(bootstrap), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                  totals.data_ptr(), u2.data_ptr(), hits.data_ptr() if n_cut else None, expsum.data_ptr(),
                                  ranked.data_ptr() if ranked is not None and ranked.numel() else None, ranked.shape[1] if ranked is not None else 0,
                                  tdev.index, ctypes.c_void_p(stream)))
    tot = totals.cpu().numpy().view(np.uint64)
    if int(tot[0, 0]) == 0xFFFFFFFFFFFFFFFF:
        raise _ffi.PmxError("pmx_enrichment: labels other than 0 (decoy), 1 (active) and 2 (not counted)")
    return Enrichment(totals=tot, u2=u2.cpu().numpy().view(np.uint64), hits=hits.cpu().numpy(), expsum=expsum.cpu().numpy(), cut_ppm=ppm, alpha=float(alpha),
                      seed=int(seed), order=ranked.cpu().numpy() if ranked is not None else None, columns=list(columns) if columns is not None else [])


def sweep(models, library, labels, weight_sets, cutoffs=(0.005, 0.01, 0.05), alpha: float = 20.0, bootstrap: int = 0, seed: int = 0, order: bool = False,
          device=None, return_scores: bool = False):
    """Calibration: every model of `models` under every weight set of `weight_sets` (dicts as `screen` takes them, None for the defaults)
    over one labelled library - one `pmx_score` per (model, weight set) into one [n_cols, n] buffer, then one `enrichment` over all
    columns. Column m * len(weight_sets) + w is named (m, w) and is bit for bit `screen(models[m], library, weights=weight_sets[w]).scores`;
    the resamples are shared, so `delta((m, w), (m2, w2), metric)` is paired. It evaluates the sets it is given and changes no score.
    (A ligand `pmx_score` reports with a non-zero status has a NaN score, which ranks as the status would.) With `return_scores` the
    result is (Enrichment, scores tensor)."""
    torch = _torch()
    lib = _ffi.load()
    models, weight_sets = list(models), list(weight_sets)
    if not models or not weight_sets or len(models) * len(weight_sets) > MAX_COLUMNS:
        raise ValueError(f"sweep: 1 to {MAX_COLUMNS} (model, weight set) columns")
    with _resident(library, device) as dlib:
        tdev = torch.device("cuda", dlib.device)
        n = len(dlib)
        scores = torch.empty((len(models) * len(weight_sets), n), dtype=torch.float32, device=tdev)
        status = torch.empty(n, dtype=torch.int32, device=tdev)
        stream = torch.cuda.current_stream(tdev).cuda_stream
        columns = []
        for m, model in enumerate(models):
            mh = device_model(model, dlib.device)
            for w, weights in enumerate(weight_sets):
                _ffi.check(lib.pmx_score(mh.handle, dlib.handle, _weights_array(weights), 0, n, scores[len(columns)].data_ptr(), status.data_ptr(), ctypes.c_void_p(stream)))
                columns.append((m, w))
        en = enrichment(scores, labels, cutoffs=cutoffs, alpha=alpha, bootstrap=bootstrap, seed=seed, order=order, columns=columns)
    return (en, scores) if return_scores else en


def score_one(model, ligand, weights: dict[str, float] | None = None, device=None) -> float:
    """`PharmacophoreModel._scoring` for one ligand: a Python float, like the reference returns."""
    packed = as_packed_library(ligand)
    if len(packed) != 1:
        raise ValueError("_scoring takes exactly one ligand")
    n, c, ncl = packed.header(0)
    if ncl == 0 and n == 0 and c > 0:
        return 0  # `GraphMatcher.run()` returns the int 0 for a ligand without clusters (graph_match.py:95-96)
    result = screen(model, packed, weights=weights, device=device, float64=True)  # (the reference returns a Python float: a float64)
    if int(result.status.cpu()[0]) != 0:
        raise ValueError(
            f"ligand outside the structural limits of the GPU engine (nodes={n}, conformers={c}); see include/pmx.h"
        )
    return float(result.scores.cpu()[0])




@dataclass
class Explanation:
    """What `explain` returns: one row per listed ligand, cut to that ligand's conformers C and tree levels nl.

    conf_max[i]        float64 [C]: per conformer the maximum over the tree's leaves (`scores` inside `_run_average`; its mean is the
                       ligand's score); NaN for a ligand with a non-zero status
    best_conformer[i]  the smallest conformer with the largest maximum (-1 with a non-zero status)
    levels[i]          int [nl]: the ligand cluster (index in the record's priority-ordered cluster list) behind each tree level
    match[i]           int [C, nl]: per conformer the key of the first leaf (in `root_tree.iteration()` order) that reaches its
                       maximum - the model cluster (index in `model.node_clusters`) each level is matched to, -1 for None; all -1 where the
                       maximum is 0 (no leaf explains it)
    status[i]          PMX_LIGAND_* as `screen` reports it
    require, exclude   the constraint it was made with (`explain`): maxima and keys are then over the qualifying leaves only; None without"""

    indices: np.ndarray
    conf_max: list
    best_conformer: np.ndarray
    levels: list
    match: list
    status: np.ndarray
    require: "tuple | None" = None  # normalised: a tuple of groups, each a sorted tuple of model cluster indices
    exclude: "tuple | None" = None  # a sorted tuple of model cluster indices

    def __len__(self) -> int:
        return len(self.indices)

    @property
    def scores(self) -> np.ndarray:
        """Per ligand the mean of `conf_max` - the ligand's score (graph_match.py:109), the constrained score of a constrained
        explanation; NaN for a ligand with a non-zero status."""
        return np.array([float(np.mean(m)) if st == 0 and m.size else (np.nan if st != 0 else 0.0) for m, st in zip(self.conf_max, self.status)])

    @property
    def max(self) -> np.ndarray:
        """Per ligand the largest conformer maximum (`GraphMatcher._run_max`, graph_match.py:111-112)."""
        return np.array([float(m.max()) if m.size else 0.0 for m in self.conf_max])

    def pairs(self, i: int, model, library, conformer: int | None = None) -> list[dict]:
        """Row i as readable pairs for one conformer (default: the best one): per tree level the ligand cluster (index, types, node count,
        centre in that conformer) and the model cluster it is matched to (index, type, centre), or None. (A packed record holds typed
        nodes, not atoms: the atom indices of a ligand cluster are those of its nodes in the `LigandGraph` the record was packed from.)"""
        from .constants import TYPE_NAMES

        packed = library if isinstance(library, PackedLibrary) else as_packed_library(library)
        c = int(self.best_conformer[i]) if conformer is None else int(conformer)
        if c < 0 or self.status[i] != 0:
            return []
        rec = packed.unpack(int(self.indices[i]))
        ends = rec["cluster_end"]
        flat = model.flat
        out = []
        for lev, lc in enumerate(self.levels[i]):
            lc = int(lc)
            s0 = int(ends[lc - 1]) if lc > 0 else 0
            s1 = int(ends[lc])
            tm = int(np.bitwise_or.reduce(rec["typemask"][s0:s1])) if s1 > s0 else 0
            centre = rec["xyz"][s0:s1, :, c].astype(np.float64).mean(axis=0) if s1 > s0 else np.zeros(3)
            m = int(self.match[i][c, lev])
            out.append(dict(
                level=lev,
                ligand_cluster=lc,
                ligand_types=[TYPE_NAMES[t] for t in range(len(TYPE_NAMES)) if tm >> t & 1],
                ligand_nodes=s1 - s0,
                ligand_center=tuple(float(x) for x in centre),
                model_cluster=None if m < 0 else m,
                model_type=None if m < 0 else flat.cluster_type[m],
                model_center=None if m < 0 else tuple(float(x) for x in flat.cluster_center[m]),
            ))
        return out


    def attribution(self, model, library, conformer: int | None = None, weights: dict[str, float] | None = None) -> "Attribution":
        """`attribute` of every row with status 0, at its best conformer (or `conformer`) under that conformer's own key: which nodes
        carry the explained maximum. `rows` of the result says which row of this explanation each of its rows is. A constrained
        explanation needs nothing more: the reported keys are attributed, and they are the qualifying leaves' keys."""
        rows, conf, keys = self._own_rows(conformer)
        out = attribute(model, library, self.indices[rows], conf, keys, weights=weights)
        out.rows = np.asarray(rows, dtype=np.int64)
        return out

    def poses(self, model, library, conformer: int | None = None, weights: dict[str, float] | None = None) -> "Alignment":
        """`align` of every row with status 0, at its best conformer (or `conformer`) under that conformer's own key: where the explained
        match puts the ligand in the pocket. `rows` of the result says which row of this explanation each of its rows is."""
        rows, conf, keys = self._own_rows(conformer)
        out = align(model, library, self.indices[rows], conf, keys, weights=weights)
        out.rows = np.asarray(rows, dtype=np.int64)
        return out

    def pose_fit(self, model, library, conformer: int | None = None, weights: dict[str, float] | None = None, **kw) -> "PoseFit":
        """`pose_fit` of every row with status 0, posed as `poses` poses it and scored in key mode under the same key: how well the
        explained match, once fitted, sits on the hotspots it was fitted to. Rows as `poses` has them."""
        rows, conf, keys = self._own_rows(conformer)
        al = align(model, library, self.indices[rows], conf, keys, weights=weights)
        return al.pose_fit(model, library, keys=keys, weights=weights, **kw)

    def hotspots(self, model, library, conformer: int | None = None, weights: dict[str, float] | None = None) -> "HotspotProfile":
        """`hotspots` of every row with status 0, at its best conformer (or `conformer`) under that conformer's own key: which model nodes
        carry the explained maximum, and the row's interaction fingerprint. `rows` of the result says which row of this explanation each
        of its rows is."""
        rows, conf, keys = self._own_rows(conformer)
        out = hotspots(model, library, self.indices[rows], conf, keys, weights=weights)
        out.rows = np.asarray(rows, dtype=np.int64)
        return out

    def _own_rows(self, conformer):
        """The rows with status 0, the conformer each is looked at (its best one, or `conformer`) and that conformer's own key."""
        rows = [i for i in range(len(self)) if self.status[i] == 0]
        conf = [int(self.best_conformer[i]) if conformer is None else int(conformer) for i in rows]
        keys = []
        for i, c in zip(rows, conf):
            m = self.match[i]
            keys.append(m[c] if 0 <= c < m.shape[0] else np.full(len(self.levels[i]), -1, np.int64))  # (not a conformer of the ligand: reported by the row's status)
        return rows, conf, keys


def normalize_constraint(require=None, exclude=None, num_clusters: int | None = None):
    """`require` (a sequence of groups, each an int or a sequence of ints) and `exclude` (a sequence of ints) as (tuple of sorted tuples,
    sorted tuple) of model cluster indices. ValueError for a negative index or, with `num_clusters`, an index outside the model; an
    empty group and a ninth group are kept as they are (`pmx_explain_constrained` refuses them)."""
    def one(v, what):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{what}: a model cluster index, not {v!r}")
        if v < 0 or (num_clusters is not None and v >= num_clusters):
            raise ValueError(f"{what}: model cluster {int(v)} is outside the model" + (f"'s {num_clusters} clusters" if num_clusters is not None else ""))
        return int(v)

    groups = []
    for g in ([] if require is None else require):
        members = [g] if isinstance(g, (int, np.integer)) else list(g)
        groups.append(tuple(sorted({one(v, "require") for v in members})))
    if exclude is not None and isinstance(exclude, (int, np.integer)):
        exclude = [exclude]
    return tuple(groups), tuple(sorted({one(v, "exclude") for v in ([] if exclude is None else exclude)}))


def _constraint_struct(groups, excluded) -> "_ffi.MatchConstraint":
    con = _ffi.MatchConstraint()
    con.n_require = len(groups)
    for g, members in enumerate(groups[: _ffi.MAX_REQUIRE_GROUPS]):
        for a in members:
            con.require[g][a // 64] |= 1 << (a % 64)
    for a in excluded:
        con.exclude[a // 64] |= 1 << (a % 64)
    return con


def key_qualifies(key, require, exclude) -> bool:
    """Does a key (a model cluster or -1 per level) hold a cluster of every group of `require` and none of `exclude` (both normalised)."""
    have = {int(m) for m in key if m >= 0}
    return all(have & set(g) for g in require) and not (have & set(exclude))


def explain(model, library, indices, weights: dict[str, float] | None = None, device=None, require=None, exclude=None) -> Explanation:
    """Per-conformer maxima and the leaf that reaches each (`pmx_explain`, csrc/pmx_explain.hip) for the library ligands `indices`
    (any order, repeats allowed, at most 65536). `library` is a `DeviceLibrary` or anything `as_packed_library` accepts. Runs on torch's
    current stream of the device and waits for it.

    `require` / `exclude`: constrained matching (`pmx_explain_constrained`). `require` is a sequence of groups, each a model cluster
    index or a sequence of them; `exclude` a sequence of indices (`PharmacophoreModel.clusters_with_nodes` makes either from hotspot
    nodes). Only leaves whose key holds a cluster of every group and none of `exclude` count: `conf_max`, `scores` and `match` are over
    those leaves. With both None the call is `pmx_explain` as before."""
    n = int(np.size(indices))
    if n > 65536:
        raise ValueError("at most 65536 ligands per explain call (PMX_EXPLAIN_MAX)")
    constraint = _constraint(require, exclude)
    with _resident(library, device) as dlib:
        return _explain_rows(model, dlib, indices, 1, weights, constraint, "pmx_explain" if constraint is None else "pmx_explain_constrained").explanation()


def _constraint(require, exclude):
    """`require` / `exclude` of `explain` and `explain_modes` normalised to (groups, excluded), None when both are None."""
    if require is None and exclude is None:
        return None
    groups, excluded = normalize_constraint(require, exclude)
    if any(a >= 128 for g in groups for a in g) or any(a >= 128 for a in excluded):
        raise _ffi.PmxError("constraint: a model has at most 128 clusters (PMX_MAX_MODEL_CLUSTERS)")
    return groups, excluded


def _explain_call(model, library: "DeviceLibrary", indices, modes: int, weights, constraint, entry: str):
    """One call of `entry` enqueued on torch's current stream of the library's device, not waited for: (idx, ligands, values, match, levels,
    best, status, stream) - the indices, and the call's device tensors as the C ABI lays them out (at least one row each)."""
    torch = _torch()
    lib = _ffi.load()
    idx = np.ascontiguousarray(np.asarray(indices, dtype=np.int64).reshape(-1))
    if (idx < 0).any():
        raise ValueError("negative ligand index")
    n = len(idx)
    mh = device_model(model, library.device)
    tdev = torch.device("cuda", library.device)
    L, CM = 20, 64  # PMX_MAX_LEVELS, PMX_MAX_CONFORMERS
    m = max(n, 1)
    rows = m if n * modes > 65536 else m * modes  # (a call the library refuses writes nothing)
    lig = torch.from_numpy(idx).to(tdev)
    values = torch.empty((rows, CM), dtype=torch.float64, device=tdev)
    match = torch.empty((rows, CM, L), dtype=torch.uint8, device=tdev)
    levels = torch.empty((m, L), dtype=torch.uint8, device=tdev)
    best = torch.empty(m, dtype=torch.int32, device=tdev)
    status = torch.empty(m, dtype=torch.int32, device=tdev)
    with torch.cuda.device(tdev):
        stream = torch.cuda.current_stream(tdev)
        con = ctypes.byref(_constraint_struct(*constraint)) if constraint is not None else None
        which = {"pmx_explain": (), "pmx_explain_constrained": (con,), "pmx_explain_modes": (con, modes)}[entry]
        _ffi.check(getattr(lib, entry)(mh.handle, library.handle, _weights_array(weights), *which, lig.data_ptr(), n, values.data_ptr(), match.data_ptr(),
                                       levels.data_ptr(), best.data_ptr(), status.data_ptr(), ctypes.c_void_p(stream.cuda_stream)))
    return idx, lig, values, match, levels, best, status, stream


def _explain_rows(model, library: "DeviceLibrary", indices, modes: int, weights, constraint, entry: str) -> "ModeSet":
    """One call of `entry` (its limits are the call's to enforce) and its rows cut to each ligand's conformers and levels, as a `ModeSet`:
    `pmx_explain` (no constraint) and `pmx_explain_constrained` (`constraint` None - a NULL constraint - or normalised (groups, excluded))
    answer with one mode, `pmx_explain_modes` with `modes`."""
    idx, _, values, match, levels, best, status, stream = _explain_call(model, library, indices, modes, weights, constraint, entry)
    stream.synchronize()
    n = len(idx)
    L, CM = 20, 64  # PMX_MAX_LEVELS, PMX_MAX_CONFORMERS
    vl, mt, lv = values.cpu().numpy().reshape(-1, modes, CM)[:n], match.cpu().numpy().reshape(-1, modes, CM, L)[:n], levels.cpu().numpy()[:n]
    st, bc = status.cpu().numpy()[:n].astype(np.int32), best.cpu().numpy()[:n].astype(np.int64)
    conf = _record_counts(library, idx, 1)
    out_vl, out_lv, out_mt = [], [], []
    for i in range(n):
        nl = int(np.count_nonzero(lv[i] != NO_LEVEL))
        C = int(conf[i]) if st[i] == 0 else 0
        out_vl.append(vl[i, :, :C].copy() if st[i] == 0 else np.full((modes, 1), np.nan))
        out_lv.append(lv[i, :nl].astype(np.int64))
        key = mt[i, :, :C, :nl].astype(np.int64)
        key[key == NO_MATCH] = -1
        out_mt.append(key)
    return ModeSet(indices=idx.astype(np.int64), modes=modes, values=out_vl, match=out_mt, levels=out_lv, best_conformer=bc, status=st,
                   require=constraint[0] if constraint is not None else None, exclude=constraint[1] if constraint is not None else None)


def concat_explanations(parts: list) -> Explanation:
    """Rows of several explanations made with one constraint, in the order given."""
    first = parts[0]
    return Explanation(indices=np.concatenate([p.indices for p in parts]), conf_max=[m for p in parts for m in p.conf_max],
                       best_conformer=np.concatenate([p.best_conformer for p in parts]), levels=[v for p in parts for v in p.levels],
                       match=[m for p in parts for m in p.match], status=np.concatenate([p.status for p in parts]),
                       require=first.require, exclude=first.exclude)


def _take_rows(ex: Explanation, rows) -> Explanation:
    rows = [int(r) for r in rows]
    return Explanation(indices=ex.indices[rows], conf_max=[ex.conf_max[r] for r in rows], best_conformer=ex.best_conformer[rows],
                       levels=[ex.levels[r] for r in rows], match=[ex.match[r] for r in rows], status=ex.status[rows],
                       require=ex.require, exclude=ex.exclude)


@dataclass
class ModeSet:
    """What `explain_modes` returns: per listed ligand and conformer the `modes` best leaves of the reference's tree - those that hold the
    conformer with a score > 0 (and qualify under `require` / `exclude`), by descending score, equal scores in `root_tree.iteration()`
    order. Row i is cut to that ligand's conformers C and tree levels nl.

    values[i]          float64 [modes, C]: the leaf totals, non-increasing along the modes; 0 where the conformer has fewer such leaves;
                       values[i][0] is `Explanation.conf_max[i]`; NaN [modes, 1] for a ligand with a non-zero status
    match[i]           int [modes, C, nl]: their keys (`Explanation.match`), all -1 where the value is 0
    levels, best_conformer, status, indices, require, exclude   as `Explanation`'s; the best conformer is mode 0's"""

    indices: np.ndarray
    modes: int
    values: list
    match: list
    levels: list
    best_conformer: np.ndarray
    status: np.ndarray
    require: "tuple | None" = None
    exclude: "tuple | None" = None

    def __len__(self) -> int:
        return len(self.indices)

    def count(self, i: int) -> np.ndarray:
        """Per conformer of row i the modes found (at most `modes`)."""
        return np.count_nonzero(np.nan_to_num(self.values[i], nan=0.0) > 0, axis=0)

    def gap(self, i: int, c: int | None = None, m: int = 0) -> float:
        """(mode m - mode m + 1) / mode m of conformer c (default: the best one): how far the next mode lies below. 1.0 when there is no
        next mode (or no mode m). The last mode asked for has no known successor: ValueError for m + 1 >= `modes`."""
        if not 0 <= m < self.modes - 1:
            raise ValueError(f"the gap behind mode {m} needs modes >= {m + 2}")
        c = int(self.best_conformer[i]) if c is None else int(c)
        if c < 0 or self.status[i] != 0:
            return float("nan")
        v, nxt = float(self.values[i][m, c]), float(self.values[i][m + 1, c])
        return 1.0 if v <= 0 or nxt <= 0 else (v - nxt) / v

    def explanation(self, m: int = 0) -> Explanation:
        """Mode m of every row as an ordinary `Explanation` (`pairs`, `attribution`): its values as `conf_max`, its keys as `match`. The
        best conformer stays mode 0's, so `pairs(i, ...)` of several m compares the modes of one conformer."""
        if not 0 <= m < self.modes:
            raise ValueError(f"mode {m} of {self.modes}")
        return Explanation(indices=self.indices, conf_max=[v[m].copy() for v in self.values], best_conformer=self.best_conformer, levels=self.levels,
                           match=[k[m] for k in self.match], status=self.status, require=self.require, exclude=self.exclude)


    def pose_search(self, model, library, pocket=None, weights: dict[str, float] | None = None, max_clashing: int = 0, min_fitted: int = 1, min_fraction: float = 0.0,
                    tolerance: float = 0.5, contact: float = 4.5, node_radius: float = 1.0, conformers: int | None = None, device=None, atoms=None) -> "PoseSearch":
        """`pose_search` of these rows over the modes already held: the values and keys are uploaded instead of explained again. `weights`
        must be the ones the modes were made with (they weigh the fit). `atoms`: the library's atom store, for the search at atom level."""
        L, CM = _MAX_LEVELS, _ffi.MAX_CONFORMERS
        n, modes = len(self), self.modes
        values = np.zeros((max(n, 1), modes, CM), np.float64)
        match = np.full((max(n, 1), modes, CM, L), NO_MATCH, np.uint8)
        for i in range(n):
            if self.status[i] != 0:
                values[i] = np.nan
                continue
            C, nl = self.values[i].shape[1], len(self.levels[i])
            values[i, :, :C] = self.values[i]
            match[i, :, :C, :nl] = np.where(self.match[i] < 0, NO_MATCH, self.match[i]).astype(np.uint8)
        status = np.ascontiguousarray(self.status, dtype=np.int32) if n else np.zeros(1, np.int32)
        idx = np.ascontiguousarray(self.indices, dtype=np.int64)
        torch = _torch()
        with _resident(library, device) as dlib:
            tdev = torch.device("cuda", dlib.device)

            def explained(lo, hi):
                hi = max(hi, lo + 1)
                return tuple(torch.from_numpy(np.ascontiguousarray(a[lo:hi])).to(tdev) for a in (values, match, status))

            return _pose_search(model, dlib, _search_pocket(model, pocket), idx, modes, weights, explained, max_clashing, min_fitted, min_fraction, tolerance, contact,
                                node_radius, conformers, atoms)


def explain_modes(model, library, indices, modes: int = 4, weights: dict[str, float] | None = None, device=None, require=None, exclude=None) -> ModeSet:
    """The `modes` (1 to 8) best binding modes per conformer of the library ligands `indices` (`pmx_explain_modes`, csrc/pmx_explain.hip):
    mode 0 is `explain`'s answer bit for bit, the others are the runners-up in the order a `ModeSet` describes. Any number of ligands
    (calls of at most 65536 // modes rows each); `library`, `require`, `exclude`, stream and waiting as `explain`."""
    modes = int(modes)
    if not 1 <= modes <= _ffi.MAX_MODES:
        raise _ffi.PmxError(f"{modes} modes (1 to {_ffi.MAX_MODES}, PMX_MAX_MODES)")
    constraint = _constraint(require, exclude)
    idx = np.asarray(indices, dtype=np.int64).reshape(-1)
    step = 65536 // modes
    with _resident(library, device) as dlib:
        parts = [_explain_rows(model, dlib, idx[lo : lo + step], modes, weights, constraint, "pmx_explain_modes") for lo in range(0, max(len(idx), 1), step)]
    return ModeSet(indices=np.concatenate([p.indices for p in parts]), modes=modes, values=[v for p in parts for v in p.values],
                   match=[m for p in parts for m in p.match], levels=[v for p in parts for v in p.levels],
                   best_conformer=np.concatenate([p.best_conformer for p in parts]), status=np.concatenate([p.status for p in parts]),
                   require=parts[0].require, exclude=parts[0].exclude)


@dataclass
class PoseSearch:
    """What `pose_search` returns: per listed hit the conformer and the binding mode to pose it in (definitions: `pmx_pose_search` in
    include/pmx.h). Among the slots (mode m < `modes`, conformer c) whose fit is OK, has `min_fitted` fitted nodes and is worth
    `min_fraction` of the hit's best leaf total: the best-scoring one that passes the clash check, else the one of smallest overlap.

    conformer[i], mode[i]   the choice, -1 and -1 where the hit has no candidate (it was not scored, scores 0, or no fit is OK)
    passes[i]               the chosen pose has at most `max_clashing` clashing points
    n_candidates[i], n_passing[i], n_dropped[i]   candidates, passing candidates, and slots left out by `min_fraction`
    value[i], fraction[i]   the chosen leaf's total, and that over the hit's best total: 1.0 where nothing was given up; NaN without a choice
    key[i]                  int [nl]: the chosen key (`Explanation.match`), all -1 without a choice
    status[i]               the hit's status as `explain` reports it
    `alignment()` and `report()` are what `align` and `clashes` answer for the chosen rows, bit for bit."""

    indices: np.ndarray
    modes: int
    conformer: np.ndarray
    mode: np.ndarray
    passes: np.ndarray
    n_candidates: np.ndarray
    n_passing: np.ndarray
    n_dropped: np.ndarray
    value: np.ndarray
    fraction: np.ndarray
    key: list
    status: np.ndarray
    poses: "Alignment"
    clash: "ClashReport"
    # (no fields - what is compared field by field stays what it was: set by `pose_search(atoms=...)` on its result)
    level = "nodes"  # "atoms": the search checked the ligands' heavy atoms, from an atom store (`pmx_pose_search_atoms`)
    gather_status = None  # atom level: int32 [n], what the store says of the chosen row (1: it has no atoms for the hit)

    def __len__(self) -> int:
        return len(self.indices)

    def alignment(self) -> "Alignment":
        """The chosen rows as an ordinary `Alignment` (`clashes(atoms=...)`, `refine`, `transform`): row i is hit i; a hit without a
        choice is a row with conformer -1 and status 4 (or 1)."""
        return self.poses

    def report(self) -> "ClashReport":
        """The `ClashReport` of the chosen rows' pharmacophore nodes - at level "atoms": of their heavy atoms -, at the search's own radius,
        tolerance and contact distance."""
        return self.clash

    def pose_fit(self, model, library, **kw) -> "PoseFit":
        """`pose_fit` of the chosen rows in key mode under the chosen keys: row i is hit i, a hit without a choice a row with status 4 (or 1)."""
        return self.poses.pose_fit(model, library, keys=self.key, **kw)

    def shape(self, reference, library=None, atoms=None, **kw) -> "ShapeReport":
        """`shape` of the chosen rows against a reference ligand (`Alignment.shape` of `alignment()`): row i is hit i, a hit without a
        choice a row with status 4 (or 1)."""
        return self.poses.shape(reference, library, atoms=atoms, **kw)

    def overlay(self, reference, library=None, atoms=None, **kw) -> "ShapeOverlay":
        """`overlay` of the chosen rows from their own motions (`Alignment.overlay` of `alignment()`): row i is hit i, a hit without a
        choice a row with status 4 (or 1)."""
        return self.poses.overlay(reference, library, atoms=atoms, **kw)


def _search_chunks(conf: np.ndarray, modes: int):
    """(lo, hi, conf_stride) of consecutive runs of hits with (hi - lo) * modes * conf_stride <= 65536, conf_stride the most conformers
    (1 to 64) of a hit of the run."""
    conf = np.clip(conf, 1, _ffi.MAX_CONFORMERS)
    lo, n = 0, len(conf)
    while lo < n:
        hi, stride = lo, 1
        while hi < n and (hi + 1 - lo) * modes * max(stride, int(conf[hi])) <= _ffi.EXPLAIN_MAX:
            stride = max(stride, int(conf[hi]))
            hi += 1
        yield lo, hi, stride
        lo = hi


def _pose_search(model, dlib: "DeviceLibrary", pocket, idx: np.ndarray, modes: int, weights, explained, max_clashing, min_fitted, min_fraction, tolerance, contact,
                 node_radius, conformers, atoms=None) -> PoseSearch:
    """`pose_search` on a resident library. `explained(lo, hi)` enqueues - or uploads - rows lo .. hi of the hits' `pmx_explain_modes` output
    and returns the device tensors (values, match, status). Every chunk is enqueued before the one wait. `atoms`: the library's atom store
    (`DeviceAtoms` / `PackedAtoms`) for the search at atom level (`pmx_pose_search_atoms`)."""
    if atoms is not None:
        if not _is_store(atoms):
            raise TypeError("pose_search: atoms is the library's atom store, a DeviceAtoms or a PackedAtoms")
        with _resident_atoms(atoms, dlib.device) as dat:
            if len(dat) != len(dlib):
                raise ValueError(f"pose_search: an atom store of {len(dat)} ligands for a library of {len(dlib)}")
            return _pose_search_on(model, dlib, pocket, idx, modes, weights, explained, max_clashing, min_fitted, min_fraction, tolerance, contact, node_radius, conformers, dat)
    return _pose_search_on(model, dlib, pocket, idx, modes, weights, explained, max_clashing, min_fitted, min_fraction, tolerance, contact, node_radius, conformers, None)


def _pose_search_on(model, dlib: "DeviceLibrary", pocket, idx: np.ndarray, modes: int, weights, explained, max_clashing, min_fitted, min_fraction, tolerance, contact,
                    node_radius, conformers, dat: "DeviceAtoms | None") -> PoseSearch:
    torch = _torch()
    lib = _ffi.load()
    if (idx < 0).any():
        raise ValueError("negative ligand index")
    if int(max_clashing) < 0 or int(min_fitted) < 1 or not 0.0 <= float(min_fraction) <= 1.0:
        raise ValueError("pose_search: max_clashing >= 0, min_fitted >= 1 and min_fraction in [0, 1]")
    if conformers is not None and not 1 <= int(conformers) <= _ffi.MAX_CONFORMERS:
        raise ValueError(f"pose_search: conformers 1 to {_ffi.MAX_CONFORMERS}")
    n = len(idx)
    m = max(n, 1)
    L, NN = _MAX_LEVELS, _MAX_NODES
    mh = device_model(model, dlib.device)
    ph = device_pocket(pocket, dlib.device)
    tdev = torch.device("cuda", dlib.device)
    conf = _record_counts(dlib, idx, 1)
    chunks = list(_search_chunks(conf if conformers is None else np.minimum(conf, int(conformers)), modes))
    with torch.cuda.device(tdev):
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=tdev)  # noqa: E731
        f64, i32, u8 = torch.float64, torch.int32, torch.uint8
        out = dict(choice=new((m, 6), i32), value=new((m, 2), f64), key=new((m, L), u8), rot=new((m, 9), f64), trans=new((m, 3), f64), fit=new((m, 8), f64),
                   node=new((m, NN), f64), count=new((m, 2), i32), levels=new((m, L), u8), summary=new((m, 4), f64), ccount=new((m, 6), i32), ppen=new((m, NN), f64),
                   patom=new((m, NN), i32), fp=new((m, _FP_WORDS), torch.int64), status=new((m,), i32))
        row_status = [new((3 if dat is not None else 2, max(hi - lo, 1)), i32) for lo, hi, _ in chunks]
        if dat is not None:  # the clash outputs in point-mode layout, per chunk: its own offsets, and room for max_atoms points per hit
            A = dat.max_atoms
            del out["ppen"], out["patom"]
            pts = [(new((hi - lo + 1,), torch.int64), new((max((hi - lo) * A, 1),), f64), new((max((hi - lo) * A, 1),), i32)) for lo, hi, _ in chunks]
            need = max([int(lib.pmx_pose_search_atoms_work_bytes(hi - lo, modes, stride, A)) for lo, hi, stride in chunks] + [256])
        else:
            need = max([int(lib.pmx_pose_search_work_bytes(hi - lo, modes, stride)) for lo, hi, stride in chunks] + [256])
        work = new((need,), u8)
        centers = mh.node_centers(model)
        stream = torch.cuda.current_stream(tdev)
        keep = []
        for k, ((lo, hi, stride), rs) in enumerate(zip(chunks, row_status)):
            lig = torch.from_numpy(np.ascontiguousarray(idx[lo:hi])).to(tdev)
            values, match, est = explained(lo, hi)
            keep.append((lig, values, match, est))
            at = lambda name: out[name][lo:].data_ptr()  # noqa: E731, B023
            if dat is not None:
                poff, ppen, patom = pts[k]
                _ffi.check(lib.pmx_pose_search_atoms(mh.handle, dlib.handle, dat.handle, _weights_array(weights), centers.data_ptr(), ph.handle, lig.data_ptr(), hi - lo,
                                                     values.data_ptr(), match.data_ptr(), est.data_ptr(), modes, stride, float(node_radius), float(tolerance), float(contact),
                                                     int(max_clashing), int(min_fitted), float(min_fraction), at("choice"), at("value"), at("key"), at("rot"), at("trans"),
                                                     at("fit"), at("node"), at("count"), at("levels"), at("summary"), at("ccount"), poff.data_ptr(), ppen.data_ptr(),
                                                     patom.data_ptr(), at("fp"), at("status"), rs.data_ptr(), work.data_ptr(), need, ctypes.c_void_p(stream.cuda_stream)))
                continue
            _ffi.check(lib.pmx_pose_search(mh.handle, dlib.handle, _weights_array(weights), centers.data_ptr(), ph.handle, lig.data_ptr(), hi - lo, values.data_ptr(),
                                           match.data_ptr(), est.data_ptr(), modes, stride, float(node_radius), float(tolerance), float(contact), int(max_clashing),
                                           int(min_fitted), float(min_fraction), at("choice"), at("value"), at("key"), at("rot"), at("trans"), at("fit"), at("node"),
                                           at("count"), at("levels"), at("summary"), at("ccount"), at("ppen"), at("patom"), at("fp"), at("status"), rs.data_ptr(),
                                           work.data_ptr(), need, ctypes.c_void_p(stream.cuda_stream)))
        stream.synchronize()
        del keep
    nn = _record_counts(dlib, idx, 0)
    h = {k: v.cpu().numpy()[:n] for k, v in out.items()}
    ast = np.concatenate([r.cpu().numpy()[0, : hi - lo] for (lo, hi, _), r in zip(chunks, row_status)] + [np.zeros(0, np.int32)]).astype(np.int32)
    cst = np.concatenate([r.cpu().numpy()[-1, : hi - lo] for (lo, hi, _), r in zip(chunks, row_status)] + [np.zeros(0, np.int32)]).astype(np.int32)
    gst = None if dat is None else np.concatenate([r.cpu().numpy()[1, : hi - lo] for (lo, hi, _), r in zip(chunks, row_status)] + [np.zeros(0, np.int32)]).astype(np.int32)
    ch, lv = h["choice"].astype(np.int64), h["levels"]
    nl = [int(np.count_nonzero(lv[i] != NO_LEVEL)) for i in range(n)]
    keys = []
    for i in range(n):
        k = h["key"][i, : nl[i]].astype(np.int64)
        k[k == NO_MATCH] = -1
        keys.append(k)
    an = [int(nn[i]) if ast[i] != 1 else 0 for i in range(n)]
    cn = [int(nn[i]) if cst[i] != 1 else 0 for i in range(n)]
    ft, cc = h["fit"], h["ccount"].astype(np.int64)
    idx = idx.astype(np.int64)
    poses = Alignment(indices=idx, conformers=ch[:, 0].copy(), rotation=h["rot"].reshape(-1, 3, 3).copy(), translation=h["trans"].copy(), rmsd=ft[:, 2].copy(),
                      rmsd_nodes=ft[:, 3].copy(), weight=ft[:, 0].copy(), sse=ft[:, 1].copy(), scale=ft[:, 4].copy(), gap=ft[:, 5].copy(),
                      node=[h["node"][i, : an[i]].copy() for i in range(n)], n_nodes=h["count"][:, 0].astype(np.int64), n_pairs=h["count"][:, 1].astype(np.int64),
                      levels=[lv[i, : nl[i]].astype(np.int64) for i in range(n)], status=ast, rows=np.arange(n, dtype=np.int64))
    if dat is not None:
        point_pen, point_atom = [], []
        for (lo, hi, _), (poff, ppen, patom) in zip(chunks, pts):
            o, pp, pa = poff.cpu().numpy(), ppen.cpu().numpy(), patom.cpu().numpy().astype(np.int64)
            point_pen += [pp[o[i]: o[i + 1]].copy() for i in range(hi - lo)]
            point_atom += [pa[o[i]: o[i + 1]].copy() for i in range(hi - lo)]
    else:
        point_pen, point_atom = [h["ppen"][i, : cn[i]].copy() for i in range(n)], [h["patom"][i, : cn[i]].astype(np.int64) for i in range(n)]
    clash = ClashReport(clearance=h["summary"][:, 0].copy(), overlap=h["summary"][:, 1].copy(), n_points=cc[:, 0].copy(), n_clashing=cc[:, 1].copy(), n_pairs=cc[:, 2].copy(),
                        n_contacts=cc[:, 3].copy(), worst=cc[:, 4:6].copy(), point_penetration=point_pen, point_atom=point_atom,
                        contact_fingerprint=h["fp"].view(np.uint64).copy(), status=cst, device=dlib.device)
    found = PoseSearch(indices=idx, modes=modes, conformer=ch[:, 0].copy(), mode=ch[:, 1].copy(), passes=ch[:, 2] != 0, n_candidates=ch[:, 3].copy(), n_passing=ch[:, 4].copy(),
                      n_dropped=ch[:, 5].copy(), value=h["value"][:, 0].copy(), fraction=h["value"][:, 1].copy(), key=keys, status=h["status"].astype(np.int32), poses=poses,
                      clash=clash)
    if dat is not None:
        found.level, found.gather_status = "atoms", gst
    return found


def _search_pocket(model, pocket):
    from .pocket import PocketAtoms

    if pocket is None:
        return model.pocket_atoms()
    return pocket if isinstance(pocket, PocketAtoms) else pocket.pocket_atoms()


def pose_search(model, library, pocket, indices, modes: int = 4, weights: dict[str, float] | None = None, require=None, exclude=None, max_clashing: int = 0,
                min_fitted: int = 1, min_fraction: float = 0.0, tolerance: float = 0.5, contact: float = 4.5, node_radius: float = 1.0,
                conformers: int | None = None, device=None, atoms=None) -> PoseSearch:
    """Per hit of `indices` the conformer and binding mode that fits the pocket (`pmx_explain_modes`, then `pmx_pose_search`,
    csrc/pmx_pose_search.hip): every conformer (the first `conformers` of each, if given) under each of its `modes` (1 to 8) best modes is
    fitted (`align`) and checked against the atoms of `pocket` (a `pocket.PocketAtoms`, a model that carries its protein, or None for
    `model`'s own) as `clashes` checks pharmacophore nodes of `node_radius` at `tolerance` and `contact`. See `PoseSearch` for the choice.
    `require` / `exclude` as `explain_modes` takes them. Any number of hits: calls of at most 65536 (hit, mode, conformer) slots each, all
    enqueued on torch's current stream of the library's device and waited for once.
    With `atoms` - the library's atom store, a `DeviceAtoms` or a `PackedAtoms` - every fit is checked on the ligand's heavy atoms with
    Bondi radii instead of its nodes (`pmx_pose_search_atoms`): `PoseSearch.level` is "atoms", `report()` the atoms' `ClashReport`, and a
    hit the store has no atoms for gets no pose."""
    modes = int(modes)
    if not 1 <= modes <= _ffi.MAX_MODES:
        raise _ffi.PmxError(f"{modes} modes (1 to {_ffi.MAX_MODES}, PMX_MAX_MODES)")
    constraint = _constraint(require, exclude)
    idx = np.ascontiguousarray(np.asarray(indices, dtype=np.int64).reshape(-1))
    with _resident(library, device) as dlib:

        def explained(lo, hi):
            _, _, values, match, _, _, status, _ = _explain_call(model, dlib, idx[lo:hi], modes, weights, constraint, "pmx_explain_modes")
            return values, match, status

        return _pose_search(model, dlib, _search_pocket(model, pocket), idx, modes, weights, explained, max_clashing, min_fitted, min_fraction, tolerance, contact,
                            node_radius, conformers, atoms)


@dataclass
class ConstrainedScreeningResult:
    """What `screen_constrained` returns: the k best ligands by constrained score, best first (ties by ascending index).

    indices        int64 [<= k]: library indices of the hits (only ligands with a constrained score > 0 are hits)
    scores         float64: their constrained scores (the mean over conformers of the best qualifying leaf)
    unconstrained  float32: their scores in the ordinary screen
    explanation    the constrained `Explanation` of the hits, in the same order
    pool           how many ligands, taken in the order of the ordinary screen, were explained under the constraint
    exact          True when no ligand outside the pool can belong to (or tie with) the hits"""

    indices: np.ndarray
    scores: np.ndarray
    unconstrained: np.ndarray
    explanation: Explanation
    pool: int
    exact: bool
    screen: "ScreeningResult | None" = None  # the ordinary screen it started from


def screen_constrained(model, library, topk: int, require=None, exclude=None, weights: dict[str, float] | None = None, pool: int | None = None,
                       max_pool: int | None = None, device=None) -> ConstrainedScreeningResult:
    """The exact top-k of the whole library by CONSTRAINED score, from one ordinary screen plus constrained explanations of a pool of its
    best ligands. A constrained maximum never exceeds the unconstrained one, so with the ligands ordered by the screen's float32 score
    (descending, ties by index, non-zero status last), u the score of the first ligand outside the pool and c_k the k-th best
    constrained score inside it, the pool's top-k is the library's as soon as c_k > float64(nextafter(float32(u), +inf)): the one-ulp step
    covers the float32 rounding of the screen's score and its summation order, the strict `>` a tie from outside. Until then the pool
    doubles (only the new ligands are explained), from `pool` (default max(4 topk, 4096)) up to the library or `max_pool`, where the
    result comes back with `exact` False."""
    topk = int(topk)
    if topk <= 0:
        raise ValueError("topk must be positive")
    groups, excluded = normalize_constraint(require, exclude)
    with _resident(library, device) as dlib:
        res = screen(model, dlib, weights=weights)
        sc, st = res.scores.cpu().numpy(), res.status.cpu().numpy()
        total = len(sc)
        rank = np.where(st != 0, -np.inf, np.nan_to_num(sc.astype(np.float64), nan=-np.inf))
        order = np.lexsort((np.arange(total), -rank))  # (the order of ScreeningResult.explain)
        n = min(total, max(4 * topk, 4096) if pool is None else max(int(pool), 1))
        if max_pool is not None:
            n = min(n, max(int(max_pool), 1))
        parts, done, con = [], 0, []
        while True:
            for lo in range(done, n, 65536):
                parts.append(explain(model, dlib, order[lo : min(lo + 65536, n)], weights=weights, require=groups, exclude=excluded))
                con.append(parts[-1].scores)
            done = n
            cs = np.nan_to_num(np.concatenate(con) if con else np.zeros(0), nan=0.0)
            hits = np.flatnonzero(cs > 0)
            best = hits[np.lexsort((order[hits], -cs[hits]))][:topk]  # rows of the pool: descending constrained score, ascending index
            if n >= total:
                exact = True
            elif len(best) < topk or st[order[n]] != 0:
                exact = st[order[n]] != 0  # (nothing scored is left outside the pool)
            else:
                u = np.float32(sc[order[n]])
                exact = bool(cs[best[-1]] > np.float64(np.nextafter(u, np.float32(np.inf))))
            if exact or (max_pool is not None and n >= int(max_pool)):
                break
            n = min(total, 2 * n if max_pool is None else min(2 * n, int(max_pool)))
        ex = concat_explanations(parts) if parts else explain(model, dlib, [], weights=weights, require=groups, exclude=excluded)
    return ConstrainedScreeningResult(indices=order[best].astype(np.int64), scores=cs[best].astype(np.float64), unconstrained=sc[order[best]].astype(np.float32),
                                      explanation=_take_rows(ex, best), pool=int(n), exact=bool(exact), screen=res if dlib is library else None)


KEY_INVALID = 4  # include/pmx.h PMX_LIGAND_KEY_INVALID




def _listed_rows(indices, conformers, keys, what: str):
    """The (ligand, conformer, key) rows of an `attribute` / `align` call as the arrays the C ABI takes: int64 indices, int64 conformers and
    uint8 keys [max(n, 1), PMX_MAX_LEVELS] with 0xFF for None (shorter keys are filled with None)."""
    idx = np.ascontiguousarray(np.asarray(indices, dtype=np.int64).reshape(-1))
    conf = np.ascontiguousarray(np.asarray(conformers, dtype=np.int64).reshape(-1))
    n = len(idx)
    if (idx < 0).any():
        raise ValueError("negative ligand index")
    if len(conf) != n or len(keys) != n:
        raise ValueError("indices, conformers and keys differ in length")
    if n > 65536:
        raise ValueError(f"at most 65536 rows per {what} call (PMX_EXPLAIN_MAX)")
    L = _MAX_LEVELS
    kb = np.full((max(n, 1), L), NO_MATCH, dtype=np.uint8)
    for i, k in enumerate(keys):
        k = np.asarray(k, dtype=np.int64).reshape(-1)
        if len(k) > L:
            raise ValueError(f"key {i} has more than {L} levels")
        if ((k < -1) | (k >= NO_LEVEL)).any():
            raise ValueError(f"key {i}: a model cluster index or -1 per level")
        kb[i, : len(k)] = np.where(k < 0, NO_MATCH, k).astype(np.uint8)
    return idx, conf, kb


def _row_call(model, library, indices, conformers, keys, what: str, device, call):
    """The part `attribute` and `align` share: the rows (`_listed_rows`) go to the resident library's device, `call(lib, mh, dlib, m, ptrs)` -
    m = max(n, 1) rows to allocate, ptrs = (ligands, conformers, keys, n, levels, status, stream) as the C ABI takes them - allocates the call's
    own outputs and invokes the C function on torch's current stream; this waits for the stream. Returns idx, conf, what `call` returned, and per
    row the levels cut to the ligand's, the node count (0 for status 1) and the status."""
    torch = _torch()
    lib = _ffi.load()
    idx, conf, kb = _listed_rows(indices, conformers, keys, what)
    n = len(idx)
    with _resident(library, device) as dlib:
        mh = device_model(model, dlib.device)
        tdev = torch.device("cuda", dlib.device)
        m = max(n, 1)
        with torch.cuda.device(tdev):
            lig = torch.from_numpy(idx).to(tdev)
            cf = torch.from_numpy(np.clip(conf, -1, 2**31 - 1).astype(np.int32)).to(tdev)
            key = torch.from_numpy(kb).to(tdev)
            levels = torch.empty((m, _MAX_LEVELS), dtype=torch.uint8, device=tdev)
            status = torch.empty(m, dtype=torch.int32, device=tdev)
            stream = torch.cuda.current_stream(tdev)
            out = call(lib, mh, dlib, m, (lig.data_ptr(), cf.data_ptr(), key.data_ptr(), n, levels.data_ptr(), status.data_ptr(), ctypes.c_void_p(stream.cuda_stream)))
            stream.synchronize()
        nn = _record_counts(dlib, idx, 0)
    lv, st = levels.cpu().numpy()[:n], status.cpu().numpy()[:n].astype(np.int32)
    out_lv = [lv[i, : int(np.count_nonzero(lv[i] != NO_LEVEL))].astype(np.int64) for i in range(n)]
    return idx.astype(np.int64), conf.astype(np.int64), out, out_lv, [int(nn[i]) if st[i] != 1 else 0 for i in range(n)], st


@dataclass
class Attribution:
    """What `attribute` returns: one row per (ligand, conformer, key), cut to that ligand's nodes n and tree levels nl (definitions:
    `pmx_attribute` in include/pmx.h).

    total[i]   float64: the leaf's total for the conformer; NaN when the row is not valid (status 4) or the ligand unsupported (status 1)
    node[i]    float64 [n]: the share of each node of the packed record, in record order; they add up to total[i]; NaN like total
    entry[i]   float32 [nl, nl]: self entries on the diagonal, pair entries above it (-1: no match), 0 elsewhere and for unmatched levels;
               also given for an invalid row
    fails[i]   int [nl, nl]: failing node pairs of each pair entry
    levels[i]  int [nl]: the ligand cluster behind each tree level
    status[i]  0, 1 (PMX_LIGAND_UNSUPPORTED) or 4 (PMX_LIGAND_KEY_INVALID)"""

    indices: np.ndarray
    conformers: np.ndarray
    total: np.ndarray
    node: list
    entry: list
    fails: list
    levels: list
    status: np.ndarray
    rows: "np.ndarray | None" = None  # `Explanation.attribution`: the explanation's row behind each row

    def __len__(self) -> int:
        return len(self.indices)

    def atom_scores(self, i: int, lig) -> np.ndarray:
        """Row i per atom of `lig` (the `LigandFeatures` the record was packed from): a node's share goes to its atoms in equal parts,
        an atom adds up what it gets from its nodes. float64 [n_atoms]; its sum is total[i]."""
        from .library import record_node_atoms

        atoms = record_node_atoms(lig)
        if len(atoms) != len(self.node[i]):
            raise ValueError(f"the ligand has {len(atoms)} nodes, row {i} has {len(self.node[i])}")
        out = np.zeros(lig.num_atoms, dtype=np.float64)
        for share, at in zip(self.node[i], atoms):
            out[list(at)] += float(share) / len(at)
        return out


def attribute(model, library, indices, conformers, keys, weights: dict[str, float] | None = None, device=None) -> Attribution:
    """Entries, total and node shares (`pmx_attribute`, csrc/pmx_rows.hip) of the leaf `keys[i]` of library ligand `indices[i]` for its
    conformer `conformers[i]`. A key is an int array with a model cluster per tree level and -1 for None - the form `Explanation.match[i][c]`
    has; shorter keys are filled with None. At most 65536 rows; any order, repeats allowed. `library` is a `DeviceLibrary` or anything
    `as_packed_library` accepts. Runs on torch's current stream of the device and waits for it."""
    torch = _torch()
    L, NN = _MAX_LEVELS, _MAX_NODES

    def call(lib, mh, dlib, m, ptrs):
        lig, cf, key, n, levels, status, stream = ptrs
        tdev = torch.device("cuda", dlib.device)
        total = torch.empty(m, dtype=torch.float64, device=tdev)
        node = torch.empty((m, NN), dtype=torch.float64, device=tdev)
        entry = torch.empty((m, L, L), dtype=torch.float32, device=tdev)
        fails = torch.empty((m, L, L), dtype=torch.int16, device=tdev)
        _ffi.check(lib.pmx_attribute(mh.handle, dlib.handle, _weights_array(weights), lig, cf, key, n, total.data_ptr(), node.data_ptr(), entry.data_ptr(),
                                     fails.data_ptr(), levels, status, stream))
        return total, node, entry, fails

    idx, conf, (total, node, entry, fails), out_lv, nn, st = _row_call(model, library, indices, conformers, keys, "attribute", device, call)
    n = len(idx)
    tt, nd, en, fl = total.cpu().numpy()[:n], node.cpu().numpy()[:n], entry.cpu().numpy()[:n], fails.cpu().numpy()[:n].view(np.uint16)
    nls = [len(v) for v in out_lv]
    return Attribution(indices=idx, conformers=conf, total=tt.copy() if n else np.zeros(0), node=[nd[i, : nn[i]].copy() for i in range(n)],
                       entry=[en[i, : nls[i], : nls[i]].copy() for i in range(n)], fails=[fl[i, : nls[i], : nls[i]].astype(np.int64) for i in range(n)],
                       levels=out_lv, status=st)


def align(model, library, indices, conformers, keys, weights: dict[str, float] | None = None, device=None) -> Alignment:
    """The rigid fit (`pmx_align`, csrc/pmx_rows.hip) of library ligand `indices[i]`'s conformer `conformers[i]` under the match `keys[i]`, rows as
    `attribute` takes them. The key need not be a leaf of the ligand's tree. At most 65536 rows; any order, repeats allowed. `library` is a
    `DeviceLibrary` or anything `as_packed_library` accepts. Runs on torch's current stream of the device and waits for it."""
    torch = _torch()

    def call(lib, mh, dlib, m, ptrs):
        lig, cf, key, n, levels, status, stream = ptrs
        tdev = torch.device("cuda", dlib.device)
        centers = mh.node_centers(model)
        rot = torch.empty((m, 3, 3), dtype=torch.float64, device=tdev)
        trans = torch.empty((m, 3), dtype=torch.float64, device=tdev)
        fit = torch.empty((m, 8), dtype=torch.float64, device=tdev)
        node = torch.empty((m, _MAX_NODES), dtype=torch.float64, device=tdev)
        count = torch.empty((m, 2), dtype=torch.int32, device=tdev)
        _ffi.check(lib.pmx_align(mh.handle, dlib.handle, _weights_array(weights), centers.data_ptr(), lig, cf, key, n, rot.data_ptr(), trans.data_ptr(),
                                 fit.data_ptr(), node.data_ptr(), count.data_ptr(), levels, status, stream))
        return rot, trans, fit, node, count

    idx, conf, (rot, trans, fit, node, count), out_lv, nn, st = _row_call(model, library, indices, conformers, keys, "align", device, call)
    n = len(idx)
    ft, nd, cn = fit.cpu().numpy()[:n], node.cpu().numpy()[:n], count.cpu().numpy()[:n].astype(np.int64)
    return Alignment(indices=idx, conformers=conf, rotation=rot.cpu().numpy()[:n].copy(), translation=trans.cpu().numpy()[:n].copy(),
                     rmsd=ft[:, 2].copy(), rmsd_nodes=ft[:, 3].copy(), weight=ft[:, 0].copy(), sse=ft[:, 1].copy(), scale=ft[:, 4].copy(), gap=ft[:, 5].copy(),
                     node=[nd[i, : nn[i]].copy() for i in range(n)], n_nodes=cn[:, 0].copy(), n_pairs=cn[:, 1].copy(), levels=out_lv, status=st)


@dataclass
class FittingHits:
    """What `ScreeningResult.fitting` returns.

    indices, scores  the first k hits of the pool whose pose passes, best first: indices in the library that was screened, and their scores
    ranks            the hit's rank in the pool (0 is the screen's best hit)
    rows             the hit's row of `poses` and `report`
    pool             the library indices of the pool, best first
    poses, report    the `Alignment` and the `ClashReport` of every posed hit of the pool (hits that were not scored have no row)"""

    indices: np.ndarray
    scores: np.ndarray
    ranks: np.ndarray
    rows: np.ndarray
    pool: np.ndarray
    poses: "Alignment"
    report: "ClashReport"
    refined: "RefinedPoses | None" = None  # `fitting(refine=True)`: the refinement of every posed hit; its motion is used where the fit failed
    fit: "PoseFit | None" = None  # `fitting(fit=True)`: the `PoseFit` (free mode) of every posed hit at the motion finally used
    shape: "ShapeReport | None" = None  # `fitting(shape=reference)`: the `ShapeReport` of every posed hit at the motion finally used
    colour: "ColourReport | None" = None  # `fitting(colour=reference)`: the `ColourReport` of every posed hit's nodes at that motion

    def __len__(self) -> int:
        return len(self.indices)


@dataclass
class HotspotProfile:
    """What `hotspots` returns: one row per (ligand, conformer, key), cut to the model's nodes Nm (definitions: `pmx_hotspots` in
    include/pmx.h).

    total[i]        float64: the leaf's total, `Attribution.total` bit for bit; NaN when the row is not valid or the ligand unsupported
    share[i]        float64 [Nm]: what each model node - each hotspot of the pocket - carries of it; they add up to total[i]; NaN like total
    terms[i], passes[i]  int [Nm]: the inner terms a node is a side of, and those within two sigma
    fingerprint     uint64 [n, 4]: bit m % 64 of word m // 64 says node m is engaged (it has terms and at least half of them pass)
    levels[i]       int [nl]: the ligand cluster behind each tree level
    status[i]       0, 1 (PMX_LIGAND_UNSUPPORTED) or 4 (PMX_LIGAND_KEY_INVALID)"""

    indices: np.ndarray
    conformers: np.ndarray
    total: np.ndarray
    share: list
    terms: list
    passes: list
    fingerprint: np.ndarray
    levels: list
    status: np.ndarray
    rows: "np.ndarray | None" = None  # `Explanation.hotspots`: the explanation's row behind each row
    device: "int | None" = None  # where `similarity` and `leaders` run

    def __len__(self) -> int:
        return len(self.indices)

    def nodes(self, i: int) -> np.ndarray:
        """The engaged model nodes of row i: the set bits of its fingerprint, ascending."""
        bits = np.unpackbits(self.fingerprint[i].view(np.uint8), bitorder="little")
        return np.flatnonzero(bits).astype(np.int64)

    def cluster_share(self, i: int, model) -> np.ndarray:
        """Row i's shares summed per model cluster (index in `model.node_clusters`): float64 [K]. A node that belongs to several clusters
        counts in each of them, so the sum over the clusters can exceed total[i]."""
        flat = model.flat
        cn = np.asarray(flat.cluster_nodes, dtype=np.uint64)
        cn = cn.reshape(cn.shape[0], -1)
        member = np.unpackbits(np.ascontiguousarray(cn).view(np.uint8), axis=1, bitorder="little")[:, : len(self.share[i])].astype(bool)
        return np.array([float(self.share[i][member[a]].sum()) for a in range(member.shape[0])])

    def usage(self) -> np.ndarray:
        """Which hotspots this list of hits lives off: the mean of share / total over the rows with status 0 and total > 0. float64 [Nm];
        zeros when there is no such row."""
        rows = [i for i in range(len(self)) if self.status[i] == 0 and self.total[i] > 0]
        if not rows:
            return np.zeros(len(self.share[0]) if len(self) else 0)
        return np.mean([self.share[i] / self.total[i] for i in rows], axis=0)

    def similarity(self, other: "HotspotProfile | None" = None) -> np.ndarray:
        """Tanimoto similarity of the fingerprints, on the GPU: float32 [n, m] against `other`'s rows (default: this profile's own)."""
        return fingerprint_similarity(self.fingerprint, None if other is None else other.fingerprint, device=self.device)

    def leaders(self, threshold: float = 0.7, max_leaders: int = _MAX_LEADERS):
        """Sphere exclusion over the rows in their order, which is the caller's ranking (`fingerprint_leaders`): (leaders, leader_of)."""
        return fingerprint_leaders(self.fingerprint, threshold=threshold, max_leaders=max_leaders, device=self.device)


@dataclass
class DiverseHits:
    """What `ScreeningResult.diverse` returns.

    indices, scores  the first k leaders of the pool, best first: indices in the library that was screened, and the hits' scores
    cluster_size     per leader the hits of the pool that joined it, itself included
    leaders          the leaders' rows in the pool
    leader_of        per hit of the pool the pool row of its leader (-1: it joined none of the k)
    pool             the pooled hits' indices, best first;  profile  their `HotspotProfile`"""

    indices: np.ndarray
    scores: np.ndarray
    cluster_size: np.ndarray
    leaders: np.ndarray
    leader_of: np.ndarray
    pool: np.ndarray
    profile: "HotspotProfile"

    def __len__(self) -> int:
        return len(self.indices)


def hotspots(model, library, indices, conformers, keys, weights: dict[str, float] | None = None, device=None) -> HotspotProfile:
    """Total, model-node shares, term counts and interaction fingerprint (`pmx_hotspots`, csrc/pmx_rows.hip) of the leaf `keys[i]` of library
    ligand `indices[i]` for its conformer `conformers[i]`, rows as `attribute` takes them. At most 65536 rows; any order, repeats allowed.
    Runs on torch's current stream of the device and waits for it."""
    torch = _torch()
    NM, FW = _MAX_MODEL_NODES, _FP_WORDS
    where = []

    def call(lib, mh, dlib, m, ptrs):
        lig, cf, key, n, levels, status, stream = ptrs
        tdev = torch.device("cuda", dlib.device)
        where.append(dlib.device)
        total = torch.empty(m, dtype=torch.float64, device=tdev)
        share = torch.empty((m, NM), dtype=torch.float64, device=tdev)
        terms = torch.empty((m, NM), dtype=torch.int32, device=tdev)
        passes = torch.empty((m, NM), dtype=torch.int32, device=tdev)
        fp = torch.empty((m, FW), dtype=torch.int64, device=tdev)
        _ffi.check(lib.pmx_hotspots(mh.handle, dlib.handle, _weights_array(weights), lig, cf, key, n, total.data_ptr(), share.data_ptr(), terms.data_ptr(),
                                    passes.data_ptr(), fp.data_ptr(), levels, status, stream))
        return total, share, terms, passes, fp

    idx, conf, (total, share, terms, passes, fp), out_lv, _, st = _row_call(model, library, indices, conformers, keys, "hotspots", device, call)
    n, nm = len(idx), int(model.flat.num_nodes)
    tt, sh = total.cpu().numpy()[:n], share.cpu().numpy()[:n]
    tc, pc = terms.cpu().numpy()[:n].view(np.uint32), passes.cpu().numpy()[:n].view(np.uint32)
    return HotspotProfile(indices=idx, conformers=conf, total=tt.copy() if n else np.zeros(0), share=[sh[i, :nm].copy() for i in range(n)],
                          terms=[tc[i, :nm].astype(np.int64) for i in range(n)], passes=[pc[i, :nm].astype(np.int64) for i in range(n)],
                          fingerprint=fp.cpu().numpy()[:n].view(np.uint64).copy().reshape(n, FW), levels=out_lv, status=st, device=where[0])


@dataclass
class LigandFingerprints:
    """What `DeviceLibrary.fingerprints` returns: one row per ligand, on the device (definitions: `pmx_library_fingerprints` in include/pmx.h).

    bits         torch.int64 [n, 4]: the 256-bit set - bit j % 64 of word j // 64 is (type pair j // 9, distance bin j % 9)
    type_counts  torch.uint8 [n, 8]: per type the nodes that carry it; column 7 is the number of nodes
    status       torch.int32 [n]: 0, 1 (PMX_LIGAND_UNSUPPORTED) or 4 (PMX_LIGAND_KEY_INVALID: not a conformer of the ligand)"""

    bits: "object"
    type_counts: "object"
    status: "object"
    first: int = 0
    device: "int | None" = None

    def __len__(self) -> int:
        return int(self.status.numel())

    def numpy(self):
        """(fingerprints uint64 [n, 4], type counts uint8 [n, 8], status int32 [n]) on the host (waits for the stream)."""
        n = len(self)
        return self.bits.cpu().numpy().view(np.uint64).reshape(n, _FP_WORDS), self.type_counts.cpu().numpy().reshape(n, 8), self.status.cpu().numpy()

    def similarity(self, other: "LigandFingerprints | None" = None) -> np.ndarray:
        """Tanimoto similarity of the rows, on the GPU (`fingerprint_similarity`): float32 [n, m] against `other`'s rows (default: these);
        at most 65536 rows a side - `similar` has no such limit."""
        return fingerprint_similarity(self.numpy()[0], None if other is None else other.numpy()[0], device=self.device)

    def leaders(self, threshold: float = 0.7, max_leaders: int = _MAX_LEADERS):
        """Sphere exclusion over the rows in their order (`fingerprint_leaders`): (leaders, leader_of); at most 65536 rows."""
        return fingerprint_leaders(self.numpy()[0], threshold=threshold, max_leaders=max_leaders, device=self.device)


@dataclass
class SimilarityResult:
    """What `similar` returns, on the device.

    scores        torch.float32 [nq, n]: row q is the Tanimoto similarity of every ligand of the library to query q
    fused         torch.float32 [n]: the maximum over the queries (MAX fusion)
    status        torch.int32 [n]: the library fingerprints' status; a ligand with a non-zero one has an empty fingerprint
    topk_scores, topk_indices   the k best of `fused` (`pmx_topk`: ties in library order), None without k
    query_indices int64 [nq] for queries named as ligands of the library itself, else None"""

    scores: "object"
    fused: "object"
    status: "object"
    topk_scores: "object | None" = None
    topk_indices: "object | None" = None
    query_indices: "np.ndarray | None" = None
    columns: "object | None" = None  # [nq + 1, n]: `scores` and `fused` as one buffer (what `enrichment` ranks)

    def ranking(self) -> list[tuple[int, float]]:
        """[(ligand index, fused similarity)] of the top-k, best first."""
        assert self.topk_scores is not None and self.topk_indices is not None
        return [(int(i), float(s)) for i, s in zip(self.topk_indices.cpu().numpy(), self.topk_scores.cpu().numpy()) if i >= 0]

    def enrichment(self, labels, **kwargs) -> "Enrichment":
        """`enrichment` of the similarities: one column per query and a last one, named "fused", for their maximum - the baseline a
        model's `ScreeningResult.enrichment` is compared with (`Enrichment.delta` is paired when both are columns of one call: `columns`
        is a float32 [nq + 1, n] buffer to put next to a model's scores). Ligands that are queries themselves (`query_indices`) are
        labelled 2, not counted: a query scores 1.0 against itself."""
        torch = _torch()
        nq, n = int(self.scores.shape[0]), int(self.scores.shape[1])
        if nq + 1 > MAX_COLUMNS:
            raise ValueError(f"enrichment of a similarity search: at most {MAX_COLUMNS - 1} queries (a column each and one for their maximum)")
        lab = _labels_tensor(labels, n, self.scores.device).clone()
        if self.query_indices is not None and len(self.query_indices):
            lab[torch.from_numpy(np.asarray(self.query_indices, dtype=np.int64)).to(lab.device)] = 2
        kwargs.setdefault("columns", list(range(nq)) + ["fused"])
        return enrichment(self.columns, lab, status=self.status, **kwargs)


def similar(library, queries=None, query_indices=None, query_conformers=None, k: int | None = 100, device=None) -> SimilarityResult:
    """Ligand-based search: which ligands of `library` look like these known binders? Every ligand's own pharmacophore fingerprint (the
    union over its conformers, `DeviceLibrary.fingerprints`, kept on a `DeviceLibrary` between calls) against 1 to 64 query fingerprints
    (`pmx_fingerprint_search`: each library fingerprint is read once), and the k best by the maximum over the queries (`pmx_topk`).

    The queries are `queries` - a `PackedLibrary`, a `DeviceLibrary` or whatever `as_packed_library` accepts, of reference ligands - or
    `query_indices` - ligands of `library` itself. `query_conformers`: per query a conformer to fingerprint it at (-1 or None: the union).
    Enqueued on torch's current stream; nothing is read back."""
    torch = _torch()
    lib = _ffi.load()
    if (queries is None) == (query_indices is None):
        raise ValueError("similar: either `queries` or `query_indices`")
    with _resident(library, device) as dlib:
        tdev = torch.device("cuda", dlib.device)
        fps = dlib.fingerprints()
        n = len(dlib)
        qidx = None
        if query_indices is not None:
            qidx = np.ascontiguousarray(np.asarray(query_indices, dtype=np.int64).reshape(-1))
            if qidx.size and (int(qidx.min()) < 0 or int(qidx.max()) >= n):
                raise IndexError(f"query_indices outside the library's {n} ligands")
            if query_conformers is None:
                qbits = fps.bits[torch.from_numpy(qidx).to(tdev)].contiguous()
            else:
                sub = dlib.select(qidx)
                try:
                    qbits = sub.fingerprints(conformers=query_conformers).bits
                finally:
                    sub.close()
        else:
            with _resident(queries, dlib.device) as qlib:
                qbits = qlib.fingerprints(conformers=query_conformers).bits
        nq = int(qbits.shape[0])
        if not 1 <= nq <= _MAX_QUERIES:
            raise ValueError(f"similar: 1 to {_MAX_QUERIES} queries, not {nq}")
        with torch.cuda.device(tdev):
            columns = torch.empty((nq + 1, n), dtype=torch.float32, device=tdev)
            stream = ctypes.c_void_p(torch.cuda.current_stream(tdev).cuda_stream)
            _ffi.check(lib.pmx_fingerprint_search(qbits.data_ptr(), nq, fps.bits.data_ptr() if n else None, n, columns.data_ptr() if n else None, n,
                                                  columns[nq].data_ptr() if n else None, dlib.device, stream))
        result = SimilarityResult(scores=columns[:nq], fused=columns[nq], status=fps.status, query_indices=qidx, columns=columns)
        if k is not None and n:
            result.topk_scores, result.topk_indices = topk(columns[nq], int(k))
    return result


def last_score_stats() -> dict:
    st = _ffi.ScoreStats()
    _ffi.check(_ffi.load().pmx_score_stats_get(ctypes.byref(st)))
    return {name: (list(getattr(st, name)) if name == "dbg" else getattr(st, name)) for name, _ in st._fields_}


def release_workspaces(device=None) -> None:
    """Free the device buffers libpmx caches between scoring calls (`pmx_release_workspaces`)."""
    _ffi.check(_ffi.load().pmx_release_workspaces(_device_index(device)))


def set_profiling(enabled: bool) -> None:
    _ffi.check(_ffi.load().pmx_set_profiling(1 if enabled else 0))
