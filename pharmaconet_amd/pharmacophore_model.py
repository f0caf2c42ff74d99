"""`PharmacophoreModel`: the `.pm` / `.json` model object and the scoring entry points.

Host-side mirror of the reference's `src/pmnet/pharmacophore_model.py`:

* `load` / `save` and the state schema follow `pharmacophore_model.py:151-204`
  (`.pm` = pickle of a builtins-only dict, `.json` = the same dict; any other
  extension raises `NotImplementedError`, `:160-161,172-173`).
* `scoring_file` / `scoring_smiles` / `scoring_pbmol` / `_scoring` keep the
  reference's names and argument meaning (`pharmacophore_model.py:60-106`).
  They return a Python float computed by the HIP engine (`pharmaconet_amd.engine`);
  there is no CPU scoring path in this package.
* `screen` is the batched form of `screening.py:46-75`: one packed library in,
  per-ligand scores (and optionally a top-k) out.

What the device consumes is `FlatModel`: dense `[Nm, Nm]` float32 edge tables
(the `model_node1.neighbor_edge_dict[model_node2]` lookup of
`match_utils.py:35-48` made positional), node types, and the cluster list in
`model.node_clusters` order (`pharmacophore_model.py:202-204`).
"""

from __future__ import annotations

import io
import json
import math
import os
import pickle
from dataclasses import dataclass
from pathlib import Path
from typing import Any

import numpy as np

from .constants import MAX_MODEL_CLUSTERS, MAX_MODEL_NODES, TYPE_ID

__all__ = ["PharmacophoreModel", "FlatModel"]


class _BuiltinsOnlyUnpickler(pickle.Unpickler):
    """A `.pm` file holds dict/list/tuple/str/int/float only (`pharmacophore_model.py:178-189`)."""

    def find_class(self, module: str, name: str):  # pragma: no cover - defensive
        raise pickle.UnpicklingError(f".pm files contain builtins only; refusing to import {module}.{name}")


@dataclass
class FlatModel:
    """Positional tables of one pharmacophore model (host arrays handed to `pmx_model_create`)."""

    node_type: np.ndarray  # u8 [Nm]       type id of each model node
    edge_mean: np.ndarray  # f32 [Nm, Nm]  distance_mean of edge (m, n), symmetric, self-loops on the diagonal
    edge_std: np.ndarray  # f32 [Nm, Nm]   distance_std
    cluster_nodes: np.ndarray  # u64 [K] (models of up to 64 nodes) or [K, ceil(Nm / 64)]: bit m % 64 of word m // 64 set <=> node m in cluster
    cluster_typemask: np.ndarray  # u8 [K] bit t set <=> type t in the cluster's stored node_types
    cluster_center: np.ndarray  # f64 [K, 3]
    cluster_size: np.ndarray  # f64 [K]
    cluster_type: tuple[str, ...]

    @property
    def num_nodes(self) -> int:
        return int(self.node_type.shape[0])

    @property
    def num_clusters(self) -> int:
        return int(self.cluster_nodes.shape[0])


def _node_masks(masks: list[int], nm: int) -> np.ndarray:
    """Python-int node sets -> the words `pmx_model_desc.cluster_nodes` holds (one per cluster up to 64 nodes)."""
    words = max(1, (nm + 63) // 64)
    out = np.array([[(m >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(words)] for m in masks], dtype=np.uint64).reshape(len(masks), words)
    return out[:, 0].copy() if words == 1 else out


def cluster_node_sets(flat: "FlatModel") -> list[int]:
    """The node set of every cluster as a Python int (bit m <=> node m), whatever the word count."""
    cn = np.asarray(flat.cluster_nodes, dtype=np.uint64).reshape(flat.num_clusters, -1)
    return [sum(int(cn[k, w]) << (64 * w) for w in range(cn.shape[1])) for k in range(cn.shape[0])]


def _flatten_state(state: dict[str, Any]) -> FlatModel:
    nodes = state["nodes"]
    edges = state["edges"]
    nm = len(nodes)
    if nm > MAX_MODEL_NODES:
        raise ValueError(f"model has {nm} nodes; this implementation supports at most {MAX_MODEL_NODES}")
    for pos, node in enumerate(nodes):
        if int(node["index"]) != pos:
            raise ValueError("model node indices must be positional (pharmacophore_model.py:193,218)")
    node_type = np.array([TYPE_ID[node["type"]] for node in nodes], dtype=np.uint8)

    mean64 = np.full((nm, nm), np.nan, dtype=np.float64)
    std64 = np.full((nm, nm), np.nan, dtype=np.float64)
    for node in nodes:
        i = int(node["index"])
        # json stores the neighbour index as str (pharmacophore_model.py:279-281)
        for nbr, edge_index in node["neighbor_edge_dict"].items():
            edge = edges[int(edge_index)]
            mean64[i, int(nbr)] = float(edge["distance_mean"])
            std64[i, int(nbr)] = float(edge["distance_std"])
    # match_utils.py:35-48 builds float32 arrays of the means / stds
    edge_mean = mean64.astype(np.float32)
    edge_std = std64.astype(np.float32)

    cluster_nodes: list[int] = []
    cluster_typemask: list[int] = []
    centers: list[tuple[float, float, float]] = []
    sizes: list[float] = []
    ctypes_: list[str] = []
    # model.node_clusters = concatenation of node_cluster_dict.values() (pharmacophore_model.py:202-204)
    for cluster_list in state["node_cluster_dict"].values():
        for cluster in cluster_list:
            mask = 0
            for index in cluster["node_indices"]:
                mask |= 1 << int(index)
            tmask = 0
            for typ in cluster["node_types"]:
                tmask |= 1 << TYPE_ID[typ]
            cluster_nodes.append(mask)
            cluster_typemask.append(tmask)
            x, y, z = cluster["center"]
            centers.append((float(x), float(y), float(z)))
            sizes.append(float(cluster["size"]))
            ctypes_.append(str(cluster["cluster_type"]))
    if len(cluster_nodes) > MAX_MODEL_CLUSTERS:
        raise ValueError(
            f"model has {len(cluster_nodes)} clusters; this implementation supports at most {MAX_MODEL_CLUSTERS}"
        )
    # every (m, n) the matcher can look up must have an edge: m in cluster a, n in cluster b, any a, b
    in_cluster = 0
    for mask in cluster_nodes:
        in_cluster |= mask
    used = [m for m in range(nm) if (in_cluster >> m) & 1]
    for m in used:
        for n in used:
            if math.isnan(mean64[m, n]):
                raise ValueError(f"model edge ({m}, {n}) is missing from neighbor_edge_dict")
    edge_mean = np.nan_to_num(edge_mean, nan=0.0)
    edge_std = np.nan_to_num(edge_std, nan=1.0)

    return FlatModel(
        node_type=node_type,
        edge_mean=np.ascontiguousarray(edge_mean),
        edge_std=np.ascontiguousarray(edge_std),
        cluster_nodes=_node_masks(cluster_nodes, nm),
        cluster_typemask=np.array(cluster_typemask, dtype=np.uint8),
        cluster_center=np.array(centers, dtype=np.float64).reshape(-1, 3),
        cluster_size=np.array(sizes, dtype=np.float64),
        cluster_type=tuple(ctypes_),
    )


def _one_packed(ligand, what: str):
    """`ligand` (anything `library.as_packed_library` accepts) as a packed library of the one ligand that `what`, a one-ligand call, takes."""
    from .library import as_packed_library

    packed = as_packed_library(ligand)
    if len(packed) != 1:
        raise ValueError(f"{what} takes exactly one ligand")
    return packed


def _outside_limits(packed) -> ValueError:
    n, c, _ = packed.header(0)
    return ValueError(f"ligand outside the structural limits of the GPU engine (nodes={n}, conformers={c}); see include/pmx.h")


def _row(result, i: int, *groups) -> dict:
    """Row i of an engine result as a dict: `groups` are (type, "field names") in the order of the keys - `float`, `int` or `bool` for a
    scalar of that type, None for the row's array as it is."""
    return {f: getattr(result, f)[i] if cast is None else cast(getattr(result, f)[i]) for cast, names in groups for f in names.split()}


def _pose_fields(pose: dict) -> dict:
    """What every call made of `scoring_pose` hands on from it."""
    return {f: pose[f] for f in ("conformer", "key", "rotation", "translation", "rmsd")}


def _points_of(ligand, conformers, level: str | None = None, packed=None):
    """(level, the keyword arguments that name the points of one row per conformer of `conformers` for the posed-row calls): the ligand's
    heavy atoms with Bondi radii ("atoms") where it has them, its record's pharmacophore nodes ("nodes") otherwise - or as `level` says."""
    if level == "atoms" or (level is None and getattr(ligand, "atom_positions", None) is not None):
        from .engine import _heavy_atoms

        points, radii = _heavy_atoms([ligand] * len(conformers), conformers)
        return "atoms", dict(points=points, point_radii=radii)
    if packed is None:
        from .library import as_packed_library

        packed = as_packed_library(ligand)
    return "nodes", dict(library=packed, indices=[0] * len(conformers), conformers=conformers)


def _posed(result, row: int, ligand, packed, c: int, ok: bool):
    """(positions, node_positions) of conformer `c` under the motion of `result`'s row: the molecule's atoms (None for a packed record, which
    holds nodes, not atoms) and the record's nodes; both None where the row is not `ok`."""
    atoms = getattr(ligand, "atom_positions", None)  # [n_atoms, C, 3] of a `Ligand` / `LigandFeatures`
    positions = result.transform(row, np.asarray(atoms, dtype=np.float64)[:, c]) if ok and atoms is not None else None
    return positions, (result.transform(row, packed.unpack(0)["xyz"][:, :, c].astype(np.float64)) if ok else None)


class PharmacophoreModel:
    """Pickle-friendly pharmacophore model (`pharmacophore_model.py:50-58`)."""

    def __init__(self):
        self._state: dict[str, Any] | None = None
        self._flat: FlatModel | None = None
        self._engine_handle = None  # device tables, created on first scoring call, never pickled

    # ------------------------------------------------------------------ I/O
    @classmethod
    def load(cls, save_path: str | Path) -> "PharmacophoreModel":
        extension = os.path.splitext(save_path)[-1]
        if extension == ".pm":
            with open(save_path, "rb") as f:
                state = _BuiltinsOnlyUnpickler(io.BytesIO(f.read())).load()
        elif extension == ".json":
            with open(save_path) as f:
                state = json.load(f)
        else:
            raise NotImplementedError
        model = cls()
        model.__setstate__(state)
        return model

    def save(self, save_path: str | Path) -> None:
        extension = os.path.splitext(save_path)[-1]
        state = self.__getstate__()
        if extension == ".pm":
            with open(save_path, "wb") as w:
                pickle.dump(state, w)
        elif extension == ".json":
            with open(save_path, "w") as w:
                json.dump(state, w, indent=2)
        else:
            raise NotImplementedError

    def __getstate__(self) -> dict[str, Any]:
        assert self._state is not None, "empty model"
        return self._state

    def __setstate__(self, state: dict[str, Any]) -> None:
        self._state = state
        self._flat = _flatten_state(state)
        self._engine_handle = None
        self._object_graph = None
        self._pocket_atoms = {}

    @classmethod
    def create(cls, pdbblock, center, hotspot_infos, resolution: float = 0.5, size: int = 64, device="auto"):
        """Hotspot density maps -> model (`pharmacophore_model.py:108-149`): same arguments as the reference;
        `hotspot_infos` = [{nci_type, hotspot_position, hotspot_score, point_map}]. The graph build of
        `utils/density_map.py` is restated in `pharmaconet_amd.model_builder`: the voxel searches of all hotspots run on the GPU
        (`device`: ordinal, "auto" = the current GPU if one is visible, None = the host loop), the rest - a few dozen nodes - on
        the host; the state is the reference's either way."""
        from .model_builder import build_model_state

        model = cls()
        auto = device == "auto"
        if auto:
            device = None
            try:
                import torch

                if torch.cuda.is_available():
                    device = torch.cuda.current_device()
            except Exception:
                device = None
        try:
            state = build_model_state(pdbblock, center, hotspot_infos, resolution, size, device=device)
        except (RuntimeError, OSError):  # (_ffi.PmxError is a RuntimeError)
            # "auto" promises a model, not a GPU: libpmx.so missing or unloadable, or maps the device search cannot take
            # (model_builder.voxel_components_device) - the host search gives the same state
            if not auto or device is None:
                raise
            state = build_model_state(pdbblock, center, hotspot_infos, resolution, size, device=None)
        model.__setstate__(state)
        return model

    # ------------------------------------------------------------ accessors
    @property
    def pdbblock(self) -> str | None:
        assert self._state is not None
        return self._state.get("pdbblock")

    @property
    def flat(self) -> FlatModel:
        assert self._flat is not None, "empty model"
        return self._flat

    @property
    def num_nodes(self) -> int:
        return self.flat.num_nodes

    @property
    def node_centers(self) -> np.ndarray:
        """float64 [Nm, 3]: `nodes[m].center`, the pharmacophore point of every model node (what `engine.align` fits ligand nodes onto)."""
        assert self._state is not None, "empty model"
        return np.array([[float(v) for v in node["center"]] for node in self._state["nodes"]], dtype=np.float64).reshape(-1, 3)

    @property
    def node_radii(self) -> np.ndarray:
        """float64 [Nm]: `nodes[m].radius`, which the reference reads as the positional sigma of the node (an edge's `distance_std` is
        sqrt(r1^2 + r2^2)) - what `engine.pose_fit` measures a posed ligand node's distance from `center` in."""
        assert self._state is not None, "empty model"
        return np.array([float(node["radius"]) for node in self._state["nodes"]], dtype=np.float64).reshape(-1)

    def pocket_atoms(self, **kw):
        """The heavy atoms of the protein this model carries (`pdbblock`) as `pocket.PocketAtoms`, what `engine.clashes` checks posed hits
        against; kept per set of arguments (`within`, `hetero`, `water`), with its device copy. ValueError when the block holds no atom."""
        from .pocket import PocketAtoms

        cache = self.__dict__.setdefault("_pocket_atoms", {})
        key = tuple(sorted(kw.items()))
        if key not in cache:
            cache[key] = PocketAtoms.from_model(self, **kw)
        return cache[key]

    # The reference's object graph (`pharmacophore_model.py:191-204,207-365`), built on first use from the state dict: code
    # written against `model.nodes / .edges / .node_dict / .node_cluster_dict / .node_clusters` keeps working. Read-only views -
    # scoring never touches them (the device tables come from `flat`).
    def _graph(self):
        g = getattr(self, "_object_graph", None)
        if g is None:
            assert self._state is not None, "empty model"
            st = self._state
            nodes = [ModelNode(self, **kw) for kw in st["nodes"]]
            g = dict(nodes=nodes)
            self._object_graph = g  # (ModelEdge / ModelNodeCluster look the nodes up through the model)
            g["edges"] = [ModelEdge(self, **kw) for kw in st["edges"]]
            for node in nodes:
                node.setup()
            g["node_dict"] = {typ: [nodes[i] for i in indices] for typ, indices in st["node_dict"].items()}
            g["node_cluster_dict"] = {typ: [ModelNodeCluster(self, **kw) for kw in lst] for typ, lst in st["node_cluster_dict"].items()}
            g["node_clusters"] = [c for lst in g["node_cluster_dict"].values() for c in lst]
        return g

    @property
    def nodes(self) -> list["ModelNode"]:
        return self._graph()["nodes"]

    @property
    def edges(self) -> list["ModelEdge"]:
        return self._graph()["edges"]

    @property
    def node_dict(self) -> dict[str, list["ModelNode"]]:
        return self._graph()["node_dict"]

    @property
    def node_cluster_dict(self) -> dict[str, list["ModelNodeCluster"]]:
        return self._graph()["node_cluster_dict"]

    @property
    def node_clusters(self) -> list["ModelNodeCluster"]:
        return self._graph()["node_clusters"]

    @property
    def num_clusters(self) -> int:
        return self.flat.num_clusters

    # -------------------------------------------------------------- scoring
    def scoring_file(
        self,
        ligand_file: str | Path,
        weights: dict[str, float] | None = None,
        num_conformers: int | None = None,
    ) -> float:
        """`pharmacophore_model.py:83-90`."""
        from .ligand import Ligand

        ligand = Ligand.load_from_file(ligand_file, num_conformers)
        return self._scoring(ligand, weights)

    def scoring_smiles(
        self,
        ligand_smiles: str,
        num_conformers: int,
        weights: dict[str, float] | None = None,
    ) -> float:
        """`pharmacophore_model.py:92-99`."""
        from .ligand import Ligand

        ligand = Ligand.load_from_smiles(ligand_smiles, num_conformers)
        return self._scoring(ligand, weights)

    def scoring_pbmol(
        self,
        ligand_pbmol,
        atom_positions,
        conformer_axis: int | None = None,
        weights: dict[str, float] | None = None,
    ) -> float:
        """`pharmacophore_model.py:60-81`."""
        from .ligand import Ligand

        ligand = Ligand(ligand_pbmol, atom_positions, conformer_axis)
        return self._scoring(ligand, weights)

    def _scoring(self, ligand, weights: dict[str, float] | None = None) -> float:
        """`pharmacophore_model.py:101-106`: GraphMatcher(self, ligand, weights).run(), on the GPU.

        `ligand` is anything `pharmaconet_amd.library.as_packed_library` accepts: a `Ligand`,
        a `LigandFeatures`, packed record bytes or a one-ligand `PackedLibrary`.
        """
        from .engine import score_one

        return score_one(self, ligand, weights)

    def clusters_with_nodes(self, nodes) -> list[int]:
        """The model clusters (indices into `node_clusters`) that contain any of the model nodes `nodes` (an index or a sequence of
        them): a ready-made require group ("any cluster that holds this hotspot node") or exclude list for `explain`."""
        flat = self.flat
        wanted = 0
        for m in ([nodes] if isinstance(nodes, (int, np.integer)) else nodes):
            if not 0 <= int(m) < flat.num_nodes:
                raise ValueError(f"model node {int(m)} is outside the model's {flat.num_nodes} nodes")
            wanted |= 1 << int(m)
        return [a for a, members in enumerate(cluster_node_sets(flat)) if members & wanted]

    def scoring_detail(self, ligand, weights: dict[str, float] | None = None, require=None, exclude=None) -> dict:
        """`_scoring` with what the score is made of: `score` (the mean of `conf_max`, graph_match.py:109), `max` (`GraphMatcher._run_max`,
        graph_match.py:111-112), `conf_max` (the per-conformer maxima whose mean is the score), `best_conformer`, `levels` and `match`
        (the key of the leaf that reaches each conformer's maximum), `pairs` (the best conformer's match, readable). Takes what
        `_scoring` takes. With `require` / `exclude` (see `engine.explain`) all of it is over the qualifying leaves: the constrained score."""
        from .engine import explain

        packed = _one_packed(ligand, "scoring_detail")
        ex = explain(self, packed, [0], weights=weights, require=require, exclude=exclude)
        if int(ex.status[0]) != 0:
            raise _outside_limits(packed)
        cm = ex.conf_max[0]
        n, c, ncl = packed.header(0)
        score = 0 if (ncl == 0 and n == 0 and c > 0) else float(np.mean(cm))  # (graph_match.py:95-96 returns the int 0)
        return dict(score=score, max=float(cm.max()) if cm.size else 0.0, conf_max=cm, best_conformer=int(ex.best_conformer[0]),
                    levels=ex.levels[0], match=ex.match[0], pairs=ex.pairs(0, self, packed))

    def _leaf(self, packed, weights, conformer, key):
        """(conformer, key) of a one-ligand call: what the caller gave, else the best conformer and that conformer's explaining leaf (`engine.explain`)."""
        if conformer is None or key is None:
            from .engine import explain

            ex = explain(self, packed, [0], weights=weights)
            if int(ex.status[0]) != 0:
                raise _outside_limits(packed)
            if conformer is None:
                conformer = int(ex.best_conformer[0])
            if key is None:
                if not 0 <= int(conformer) < ex.match[0].shape[0]:
                    raise ValueError(f"the ligand has {ex.match[0].shape[0]} conformers")
                key = ex.match[0][int(conformer)]
        return int(conformer), key

    def _leaf_call(self, call, ligand, what, weights, conformer, key):
        """(packed, conformer, key, the one row of `call` - `attribute`, `hotspots` or `align` - at that leaf) for `ligand`."""
        packed = _one_packed(ligand, what)
        conformer, key = self._leaf(packed, weights, conformer, key)
        out = call(self, packed, [0], [conformer], [key], weights=weights)
        if int(out.status[0]) == 1:
            raise _outside_limits(packed)
        return packed, conformer, np.asarray(key, dtype=np.int64), out

    def scoring_attribution(self, ligand, weights: dict[str, float] | None = None, conformer: int | None = None, key=None) -> dict:
        """Which nodes of one ligand carry a leaf's total (`engine.attribute`): by default the explaining leaf of the best conformer, else
        `conformer` and / or `key` (a model cluster or -1 per tree level). `conformer`, `key`, `levels`, `total`, `node` (share per node of the
        packed record), `entry`, `fails` and `status` (0, or 4 when the key is not a leaf of the ligand's tree for that conformer: total
        and node are then NaN, `entry` says which pair stands in the way). Takes what `_scoring` takes."""
        from .engine import attribute

        _, conformer, key, at = self._leaf_call(attribute, ligand, "scoring_attribution", weights, conformer, key)
        return dict(conformer=conformer, key=key, **_row(at, 0, (None, "levels"), (float, "total"), (None, "node entry fails"), (int, "status")))

    def scoring_hotspots(self, ligand, weights: dict[str, float] | None = None, conformer: int | None = None, key=None) -> dict:
        """Which model nodes - hotspots of the pocket - carry a leaf's total for one ligand (`engine.hotspots`): by default the explaining leaf
        of the best conformer, else `conformer` and / or `key` (a model cluster or -1 per tree level). `conformer`, `key`, `levels`, `total`,
        `share` (per model node), `terms`, `passes`, `fingerprint` (uint64 [4]), `nodes` (the engaged model nodes) and `status` (0, or 4 when
        the key is not a leaf of the ligand's tree for that conformer: total and share are then NaN). Takes what `_scoring` takes."""
        from .engine import hotspots

        _, conformer, key, hs = self._leaf_call(hotspots, ligand, "scoring_hotspots", weights, conformer, key)
        return dict(conformer=conformer, key=key, **_row(hs, 0, (None, "levels"), (float, "total"), (None, "share terms passes fingerprint")), nodes=hs.nodes(0),
                    status=int(hs.status[0]))

    def scoring_pose(self, ligand, weights: dict[str, float] | None = None, conformer: int | None = None, key=None) -> dict:
        """One ligand put into the pocket (`engine.align`): by default its best conformer under the explaining leaf's match, else `conformer`
        and / or `key` (a model cluster or -1 per tree level; it need not be a leaf of the tree). `positions` [n_atoms, 3] are the
        conformer's atom positions after the fit (None when `ligand` is a packed record, which holds nodes, not atoms), `node_positions` [n, 3]
        those of the record's nodes; `rotation`, `translation`, `rmsd`, `rmsd_nodes`, `weight`, `sse`, `scale`, `gap`, `node`, `n_nodes`,
        `n_pairs`, `levels` and `status` as `engine.Alignment` has them, with `conformer` and `key`. Takes what `_scoring` takes."""
        from .engine import align

        packed, conformer, key, al = self._leaf_call(align, ligand, "scoring_pose", weights, conformer, key)
        positions, node_positions = _posed(al, 0, ligand, packed, conformer, int(al.status[0]) == 0)
        return dict(conformer=conformer, key=key, positions=positions, node_positions=node_positions,
                    **_row(al, 0, (None, "rotation translation"), (float, "rmsd rmsd_nodes weight sse scale gap"), (None, "node"), (int, "n_nodes n_pairs"), (None, "levels"),
                           (int, "status")))

    def scoring_pose_search(self, ligand, modes: int = 4, weights: dict[str, float] | None = None, pocket=None, level: str = "nodes", **kw) -> dict:
        """One ligand put into the pocket in the conformer and binding mode that fits it (`engine.pose_search`), the one-ligand form beside
        `scoring_pose`: every conformer under each of its `modes` best modes is fitted and checked against the protein's atoms (`pocket`, default
        `pocket_atoms()`), and the best-scoring pose that passes is returned - or, where none passes, the one of smallest overlap, the start
        to give `scoring_refine`. `positions` and `node_positions` as `scoring_pose` returns them, with `conformer`, `mode`, `key`, `passes`,
        `n_candidates`, `n_passing`, `value`, `fraction` (of the ligand's best leaf total), `rotation`, `translation`, `rmsd`, `rmsd_nodes`,
        `n_nodes`, `n_clashing`, `overlap`, `clearance` and `status`; conformer -1 and positions None when the ligand has no pose at all.
        Further arguments (`require`, `exclude`, `max_clashing`, `min_fitted`, `min_fraction`, `tolerance`, `contact`, `node_radius`) as
        `engine.pose_search`. Takes what `_scoring` takes. With `level="atoms"` the search checks the ligand's heavy atoms instead of its nodes
        (`engine.pose_search(atoms=...)`; `ligand` must then carry its atoms: a `Ligand` / `LigandFeatures`); the result says which `level` it is."""
        from .engine import pose_search

        packed = _one_packed(ligand, "scoring_pose_search")
        if level not in ("nodes", "atoms"):
            raise ValueError("level: 'nodes' or 'atoms'")
        if level == "atoms":
            from .atoms import PackedAtoms

            mol = getattr(ligand, "features", ligand) if not hasattr(ligand, "atom_positions") else ligand
            if not hasattr(mol, "atom_positions"):
                raise ValueError("scoring_pose_search(level='atoms'): the ligand has no atoms (a packed record); give the molecule")
            kw = dict(kw, atoms=PackedAtoms.for_library([mol], packed))
        ps = pose_search(self, packed, self.pocket_atoms() if pocket is None else pocket, [0], modes=modes, weights=weights, **kw)
        if int(ps.status[0]) != 0:
            raise _outside_limits(packed)
        al, rep, c = ps.alignment(), ps.report(), int(ps.conformer[0])
        positions, node_positions = _posed(al, 0, ligand, packed, c, c >= 0)
        return dict(conformer=c, **_row(ps, 0, (int, "mode"), (None, "key"), (bool, "passes"), (int, "n_candidates n_passing"), (float, "value fraction")),
                    positions=positions, node_positions=node_positions, **_row(al, 0, (None, "rotation translation"), (float, "rmsd rmsd_nodes"), (int, "n_nodes")),
                    **_row(rep, 0, (int, "n_clashing"), (float, "overlap clearance")), status=int(al.status[0]), level=ps.level)

    def scoring_clash(self, ligand, conformer: int | None = None, key=None, weights: dict[str, float] | None = None, pocket=None, **kw) -> dict:
        """One ligand fitted into the pocket (`scoring_pose`) and its pose checked against the protein's atoms (`engine.clashes`): the ligand's own
        heavy atoms with Bondi radii when `ligand` has them (a `Ligand` / `LigandFeatures`; `level` is "atoms"), the record's pharmacophore
        nodes otherwise ("nodes"). `pocket`: a `pocket.PocketAtoms` (default: `pocket_atoms()`, the protein this model carries). Returns
        `scoring_pose`'s `conformer`, `key`, `rotation`, `translation`, `rmsd` with `level`, `clearance`, `overlap`, `n_points`, `n_clashing`,
        `n_pairs`, `n_contacts`, `worst` (point, atom), `worst_atom` (its label), `point_penetration`, `point_atom`, `contact_fingerprint`,
        `residues` (the touched residues), `ok` and `status`. Further arguments (`tolerance`, `contact`, `node_radius`) as `engine.clashes`."""
        from .engine import clashes

        pocket = self.pocket_atoms() if pocket is None else pocket
        pose = self.scoring_pose(ligand, weights=weights, conformer=conformer, key=key)
        level, source = _points_of(ligand, [pose["conformer"]])
        rep = clashes(pocket, rotation=[pose["rotation"]], translation=[pose["translation"]], **source, **kw)
        return dict(_pose_fields(pose), level=level, **_row(rep, 0, (float, "clearance overlap"), (int, "n_points n_clashing n_pairs n_contacts")),
                    worst=tuple(int(v) for v in rep.worst[0]), worst_atom=rep.atom_label(0, pocket), **_row(rep, 0, (None, "point_penetration point_atom contact_fingerprint")),
                    residues=rep.residues(0, pocket), ok=bool(rep.ok()[0]), status=int(rep.status[0]))

    def scoring_refine(self, ligand, conformer: int | None = None, key=None, weights: dict[str, float] | None = None, pocket=None, **kw) -> dict:
        """One ligand fitted into the pocket (`scoring_pose`) and its pose moved out of the protein's atoms (`engine.refine`), the one-ligand
        form beside `scoring_clash`: the ligand's own heavy atoms with Bondi radii are the points and the anchors when `ligand` has them
        (`level` "atoms"), the record's pharmacophore nodes otherwise ("nodes"). Returns `conformer`, `key`, `level`, the fitted `rotation`
        and `translation`, the refined `refined_rotation` and `refined_translation`, `overlap_start`, `overlap`, `restraint_energy`,
        `anchor_rmsd`, `angle`, `shift`, `iterations`, `accepted`, `stop`, `n_pairs`, `status`, and `ok`: whether the refined pose passes
        `engine.clashes` at the same tolerance. Further arguments (`restraint`, `max_iter`, `ftol`, `tolerance`, `node_radius`) as
        `engine.refine`."""
        from .engine import clashes, refine

        pocket = self.pocket_atoms() if pocket is None else pocket
        pose = self.scoring_pose(ligand, weights=weights, conformer=conformer, key=key)
        level, source = _points_of(ligand, [pose["conformer"]])
        ref = refine(pocket, rotation=[pose["rotation"]], translation=[pose["translation"]], **source, **kw)
        check = {name: kw[name] for name in ("tolerance", "node_radius", "device") if name in kw}
        rep = clashes(pocket, rotation=ref.rotation, translation=ref.translation, **source, **check)
        return dict(conformer=pose["conformer"], key=pose["key"], level=level, rotation=pose["rotation"], translation=pose["translation"],
                    refined_rotation=ref.rotation[0], refined_translation=ref.translation[0],
                    **_row(ref, 0, (float, "overlap_start overlap restraint_energy anchor_rmsd angle shift"), (int, "iterations accepted stop n_pairs status")), ok=bool(rep.ok()[0]))

    def _fitted_and_refined(self, pose, head: dict, one, refine: bool, pocket, source: dict, kw: dict) -> dict:
        """`head` and `one(rotation, translation)`'s fields at the fitted motion of `pose`; with `refine` the same fields under `refined` at the
        motion `engine.refine` ends at from there (the points `source` names; `kw` its further arguments), with that motion and `stop`."""
        from .engine import refine as refine_poses

        out = dict(head, **one(pose["rotation"], pose["translation"]))
        if refine:
            ref = refine_poses(self.pocket_atoms() if pocket is None else pocket, rotation=[pose["rotation"]], translation=[pose["translation"]], **source, **kw)
            out["refined"] = dict(refined_rotation=ref.rotation[0], refined_translation=ref.translation[0], stop=int(ref.stop[0]), **one(ref.rotation[0], ref.translation[0]))
        elif kw:
            raise ValueError(f"{sorted(kw)}: arguments of the refinement, which is off (refine=True)")
        return out

    def scoring_shape(self, ligand, reference, conformer: int | None = None, key=None, refine: bool = False, weights: dict[str, float] | None = None, pocket=None,
                      node_radius: float = 1.0, cover: float = 2.0, **kw) -> dict:
        """One ligand fitted into the pocket (`scoring_pose`) and its pose compared with a known ligand (`engine.shape`; `reference` a
        `shape.ReferenceLigand` in the pocket's frame), the one-ligand form beside `scoring_clash`: the ligand's own heavy atoms with Bondi
        radii are the points when `ligand` has them (`level` "atoms"), the record's pharmacophore nodes, each of `node_radius`, otherwise
        ("nodes"). Returns `conformer`, `key`, `rotation`, `translation`, `rmsd` of the pose, `level`, and `overlap`, `self_overlap`,
        `reference_overlap`, `tanimoto`, `reference_fraction`, `fit_fraction`, `rms_to_reference`, `rms_from_reference`, `rmsd_in_order`,
        `n_points`, `n_covered`, `n_reference_covered`, `point_distance`, `point_reference_atom`, `reference_distance`, `reference_point`
        and `status`. With `refine`, the pose is also moved out of the protein's atoms (`engine.refine` on the same points; `pocket`
        defaults to `pocket_atoms()`, further arguments as `engine.refine`) and `refined` holds the same fields for the refined motion,
        with `refined_rotation`, `refined_translation` and `stop`."""
        from .engine import shape

        pose = self.scoring_pose(ligand, weights=weights, conformer=conformer, key=key)
        level, source = _points_of(ligand, [pose["conformer"]])
        source["node_radius"] = node_radius

        def one(rotation, translation):
            sh = shape(reference, rotation=[rotation], translation=[translation], cover=cover, **source)
            return _row(sh, 0, (float, "overlap self_overlap reference_overlap tanimoto reference_fraction fit_fraction rms_to_reference rms_from_reference rmsd_in_order"),
                        (int, "n_points n_covered n_reference_covered"), (None, "point_distance point_reference_atom reference_distance reference_point"), (int, "status"))

        return self._fitted_and_refined(pose, dict(_pose_fields(pose), level=level), one, refine, pocket, source, kw)

    def scoring_colour(self, ligand, reference, conformer: int | None = None, key=None, weights: dict[str, float] | None = None, cover: float = 2.0) -> dict:
        """One ligand fitted into the pocket (`scoring_pose`) and its pharmacophore nodes compared with a known ligand's typed features
        (`engine.colour`; `reference` a `shape.ColourFeatures`, or a `ReferenceLigand` that carries one, in the pocket's frame), the
        one-ligand form beside `scoring_shape`. Returns `conformer`, `key`, `rotation`, `translation`, `rmsd` of the pose, and `overlap`,
        `self_overlap`, `reference_overlap`, `tanimoto`, `reference_fraction`, `fit_fraction`, `rms_matched`, `by_type` (a dict keyed by type
        name), `n_nodes`, `n_matched`, `n_reference_features`, `n_reference_matched`, `node_overlap`, `node_distance`, `node_feature`,
        `feature_distance`, `feature_node`, `matched_fingerprint` and `status`. Points and types only: no directions."""
        from .engine import colour
        from .library import as_packed_library

        pose = self.scoring_pose(ligand, weights=weights, conformer=conformer, key=key)
        rep = colour(reference, as_packed_library(ligand), [0], [pose["conformer"]], [pose["rotation"]], [pose["translation"]], cover=cover)
        return dict(_pose_fields(pose), by_type=rep.by_type(0),
                    **_row(rep, 0, (float, "overlap self_overlap reference_overlap tanimoto reference_fraction fit_fraction rms_matched"),
                           (int, "n_nodes n_matched n_reference_features n_reference_matched status"),
                           (None, "node_overlap node_distance node_feature feature_distance feature_node matched_fingerprint")))

    def scoring_overlay(self, ligand, reference, starts: int = 4, level: str = "atoms", weights: dict[str, float] | None = None, **kw) -> dict:
        """One ligand overlaid on a known ligand (`engine.overlay`; `reference` a `shape.ReferenceLigand` in the pocket's frame), the
        one-ligand form beside `scoring_shape`. With `starts=4` every conformer is run from the four inertial starts - no pharmacophore fit
        is involved - and the conformer and start of highest final Tanimoto are kept (the lower among equals); with `starts=0` the fitted
        pose of `scoring_pose` is moved to its nearest shape match. `level` "atoms": the ligand's heavy atoms with Bondi radii (a `Ligand` /
        `LigandFeatures`); "nodes": the record's pharmacophore nodes. Returns `conformer`, `start`, `level`, `rotation`, `translation`,
        `positions` (all the molecule's atoms, posed; None for a packed record), `node_positions`, `overlap_start`, `overlap`,
        `self_overlap`, `reference_overlap`, `tanimoto_start`, `tanimoto`, `angle`, `shift`, `iterations`, `accepted`, `stop`, `n_points`
        and `status`. Further arguments (`node_radius`, `ftol`, `max_iter`) as `engine.overlay`."""
        from .engine import overlay

        if level not in ("nodes", "atoms"):
            raise ValueError("level: 'nodes' or 'atoms'")
        if starts not in (0, 4):
            raise ValueError("starts: 0 or 4")
        packed = _one_packed(ligand, "scoring_overlay")
        if level == "atoms" and getattr(ligand, "atom_positions", None) is None:
            raise ValueError("scoring_overlay(level='atoms'): the ligand has no atoms (a packed record); give the molecule, or level='nodes'")
        if starts:
            conf = list(range(int(packed.header(0)[1])))
            motion = {}
        else:
            pose = self.scoring_pose(ligand, weights=weights)
            conf = [pose["conformer"]]
            motion = dict(rotation=[pose["rotation"]], translation=[pose["translation"]])
        ov = overlay(reference, starts=starts, **_points_of(ligand, conf, level, packed)[1], **motion, **kw)
        value = np.where(np.isnan(ov.tanimoto), -np.inf, ov.tanimoto)
        r = int(np.argmax(value))  # (the first among equals)
        c = int(conf[r])
        positions, node_positions = _posed(ov, r, ligand, packed, c, int(ov.status[r]) == 0)
        return dict(conformer=c, start=int(ov.start[r]), level=level, rotation=ov.rotation[r], translation=ov.translation[r], positions=positions, node_positions=node_positions,
                    **_row(ov, r, (float, "overlap_start overlap self_overlap reference_overlap tanimoto_start tanimoto angle shift"), (int, "iterations accepted stop n_points status")))

    def scoring_pose_fit(self, ligand, conformer: int | None = None, key=None, refine: bool = False, free: bool = False, weights: dict[str, float] | None = None,
                         pocket=None, centers=None, sigmas=None, **kw) -> dict:
        """One ligand fitted into the pocket (`scoring_pose`) and its pose scored in place (`engine.pose_fit`): how well its pharmacophore
        nodes sit on the hotspots, in key mode under the pose's own key (with `free`, against every hotspot of matching type). Returns
        `conformer`, `key`, `rotation`, `translation`, `rmsd` of the pose and `fit`, `ideal`, `fraction`, `best_fit`, `best_fraction`,
        `n_nodes`, `n_pairs`, `n_in_place`, `n_passing`, `node_fit`, `node_z2`, `node_target`, `hotspot_z2`, `hotspot_node`, `occupied`
        (the model nodes some pair passes at), `coverage` and `status`. With `refine`, the pose is also moved out of the protein's atoms
        (`engine.refine` on the record's nodes; `pocket` defaults to `pocket_atoms()`, further arguments as `engine.refine`) and `refined`
        holds the same fields for the refined motion, with `refined_rotation`, `refined_translation` and `stop`: what the refinement cost
        is `fraction` against `refined["fraction"]`."""
        from .engine import pose_fit
        from .library import as_packed_library

        packed = as_packed_library(ligand)
        pose = self.scoring_pose(ligand, weights=weights, conformer=conformer, key=key)
        c, keys = pose["conformer"], (None if free else [pose["key"]])

        def one(rotation, translation):
            pf = pose_fit(self, packed, [0], [c], [rotation], [translation], keys=keys, weights=weights, centers=centers, sigmas=sigmas)
            return dict(_row(pf, 0, (float, "fit ideal fraction best_fit best_fraction"), (int, "n_nodes n_pairs n_in_place n_passing"),
                             (None, "node_fit node_z2 node_target hotspot_z2 hotspot_node")), occupied=pf.occupied(0), coverage=pf.coverage(0, self, weights), status=int(pf.status[0]))

        return self._fitted_and_refined(pose, _pose_fields(pose), one, refine, pocket, dict(library=packed, indices=[0], conformers=[c]), kw)

    def explain(self, library, indices, weights: dict[str, float] | None = None, **kwargs):
        """Per-conformer maxima and explaining matches of library ligands `indices` (`engine.explain`)."""
        from .engine import explain

        return explain(self, library, indices, weights=weights, **kwargs)

    def scoring_modes(self, ligand, modes: int = 4, weights: dict[str, float] | None = None, require=None, exclude=None) -> dict:
        """`scoring_detail` with the runners-up: per conformer the `modes` best leaves of one ligand's tree (`engine.explain_modes`). `values`
        [modes, C] and `match` [modes, C, nl] (mode 0 is `scoring_detail`'s `conf_max` and `match`), `count` [C] the modes found, `best_conformer`,
        `levels`, and `pairs`: per mode found at the best conformer its readable match. Takes what `_scoring` takes."""
        from .engine import explain_modes

        packed = _one_packed(ligand, "scoring_modes")
        ms = explain_modes(self, packed, [0], modes=modes, weights=weights, require=require, exclude=exclude)
        if int(ms.status[0]) != 0:
            raise _outside_limits(packed)
        c = int(ms.best_conformer[0])
        found = int(ms.count(0)[c]) if ms.values[0].shape[1] else 0
        return dict(values=ms.values[0], match=ms.match[0], count=ms.count(0), best_conformer=c, levels=ms.levels[0],
                    pairs=[ms.explanation(m).pairs(0, self, packed) for m in range(found)])

    def explain_modes(self, library, indices, modes: int = 4, weights: dict[str, float] | None = None, **kwargs):
        """The `modes` best binding modes per conformer of library ligands `indices` (`engine.explain_modes`)."""
        from .engine import explain_modes

        return explain_modes(self, library, indices, modes=modes, weights=weights, **kwargs)

    def screen_constrained(self, library, topk: int, require=None, exclude=None, weights: dict[str, float] | None = None, **kwargs):
        """The exact top-k by constrained score (`engine.screen_constrained`)."""
        from .engine import screen_constrained

        return screen_constrained(self, library, topk, require=require, exclude=exclude, weights=weights, **kwargs)

    def screen(self, library, weights: dict[str, float] | None = None, topk: int | None = None, **kwargs):
        """Batched `screening.py:46-75`: score every ligand of a packed library on the GPU.

        Returns a `ScreeningResult` (per-ligand float32 scores in library order; with `topk`,
        also the k best `(index, score)` in the order `screening.py:70` would list them)."""
        from .engine import screen

        return screen(self, library, weights=weights, topk=topk, **kwargs)

    def sweep(self, library, labels, weight_sets, **kwargs):
        """This model under each of `weight_sets` over a labelled library: the `Enrichment` of `engine.sweep([self], ...)`, one column per set."""
        from .engine import sweep

        return sweep([self], library, labels, weight_sets, **kwargs)


class ModelNodeCluster:
    """`pharmacophore_model.py:207-246` (a view; `get_kwargs()` gives back the state entry)."""

    def __init__(self, graph, cluster_type, node_indices, node_types, center, size):
        self.type = cluster_type
        self.nodes = {graph.nodes[int(i)] for i in node_indices}
        self.node_indices = {int(i) for i in node_indices}
        self.node_types = set(node_types)
        self.center = tuple(center)
        self.size = size

    def __repr__(self):
        return f"ModelCluster({self.type})[{self.nodes}]"

    def get_kwargs(self):
        return dict(cluster_type=self.type, node_indices=tuple(self.node_indices), node_types=tuple(self.node_types), center=self.center, size=self.size)


class ModelNode:
    """`pharmacophore_model.py:249-320`."""

    def __init__(self, graph, index, type, interaction_type, hotspot_position, score, center, radius, neighbor_edge_dict, overlapped_nodes):
        self.graph = graph
        self.index = int(index)
        self.type = type
        self.interaction_type = interaction_type
        self.hotspot_position = tuple(hotspot_position)
        self.score = score
        self.center = tuple(center)
        self.radius = radius
        self._neighbor_edge_dict = {int(k): int(v) for k, v in neighbor_edge_dict.items()}  # (.json keys are strings, :279)
        self._overlapped_nodes = [int(i) for i in overlapped_nodes]
        self.neighbor_edge_dict = {}
        self.overlapped_nodes = []

    def setup(self):
        self.neighbor_edge_dict = {self.graph.nodes[n]: self.graph.edges[e] for n, e in self._neighbor_edge_dict.items()}
        self.overlapped_nodes = [self.graph.nodes[i] for i in self._overlapped_nodes]

    def __hash__(self):
        return self.index

    def __eq__(self, other):
        return self is other

    def __repr__(self):
        return f"ModelNode({self.index})[{self.interaction_type}]"

    def get_kwargs(self):
        return dict(index=self.index, type=self.type, interaction_type=self.interaction_type, hotspot_position=self.hotspot_position,
                    score=self.score, center=self.center, radius=self.radius, neighbor_edge_dict=dict(self._neighbor_edge_dict),
                    overlapped_nodes=list(self._overlapped_nodes))


class ModelEdge:
    """`pharmacophore_model.py:323-365`."""

    def __init__(self, graph, index, node_indices, edge_type, distance_mean, distance_std):
        self.graph = graph
        self.index = int(index)
        self.node_indices = (int(node_indices[0]), int(node_indices[1]))
        self.nodes = (graph.nodes[self.node_indices[0]], graph.nodes[self.node_indices[1]])
        self.type = tuple(edge_type)
        self.distance_mean = distance_mean
        self.distance_std = distance_std

    def __hash__(self):
        return self.index

    def __eq__(self, other):
        return self is other

    def __repr__(self):
        return f"ModelEdge({self.node_indices[0]},{self.node_indices[1]})[{self.type[0]},{self.type[1]}]"

    def get_kwargs(self):
        return dict(index=self.index, node_indices=self.node_indices, edge_type=self.type, distance_mean=self.distance_mean, distance_std=self.distance_std)
