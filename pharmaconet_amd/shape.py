"""The reference ligand posed hits are compared with: the known binder of a structure-based screen, as atoms in the pocket's frame.

`ReferenceLigand` is what `engine.shape` takes - positions and radii, made from arrays, from atomic numbers, from a PDB file, or from any
posed set of points (a hit's own fitted pose, to compare the other hits with). The overlap itself is `pmx_pose_shape` (include/pmx.h).
`ColourFeatures` is what `engine.colour` and `engine.combo_overlay` take - the same ligand's typed pharmacophore features (`pmx_pose_colour`,
`pmx_combo_overlay`); a `ReferenceLigand` can carry one as its `colour`.
"""

from __future__ import annotations

import os
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

from .constants import DEFAULT_WEIGHTS, MAX_LIGAND_NODES, NUM_TYPES, TYPE_ID, TYPE_NAMES, weights_vector
from .pocket import atomic_number_radii, element_radii, parse_pdb_atoms

MAX_ATOMS = 256  # PMX_MAX_LIGAND_ATOMS
MAX_FEATURES = MAX_LIGAND_NODES  # a colour reference holds at most as many features as a record has nodes


def _posed(xyz, rotation, translation) -> np.ndarray:
    """float32 points under a motion, by the posed point of include/pmx.h (float64, every operation rounded), rounded to float32 once."""
    x = np.asarray(xyz, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    R = np.asarray(rotation, dtype=np.float64).reshape(3, 3)
    t = np.asarray(translation, dtype=np.float64).reshape(3)
    return np.stack([((R[k, 0] * x[:, 0] + R[k, 1] * x[:, 1]) + R[k, 2] * x[:, 2]) + t[k] for k in range(3)], axis=1).astype(np.float32)


def type_masks(types, check: bool = True) -> np.ndarray:
    """uint8 masks (bit t is type t of `constants.TYPE_NAMES`) from a sequence of type names (several of one feature joined by `|`), of type
    ids 0 .. 6, or - a uint8 array - of masks as they are. A name that is no type is refused by name, a mask above 127 is refused unless `check` is off (a row of `engine.colour`
    with such a mask is reported by its status)."""
    if isinstance(types, np.ndarray) and types.dtype == np.uint8:
        masks = types.reshape(-1).astype(np.int64)
    else:
        masks = []
        for v in types:
            if isinstance(v, str):
                mask = 0
                for name in v.split("|"):
                    if name.strip() not in TYPE_ID:
                        raise ValueError(f"{name.strip()!r} is no pharmacophore type: one of {', '.join(TYPE_NAMES)}")
                    mask |= 1 << TYPE_ID[name.strip()]
                masks.append(mask)
            else:
                if not 0 <= int(v) < NUM_TYPES:
                    raise ValueError(f"type id {int(v)}: 0 to {NUM_TYPES - 1}")
                masks.append(1 << int(v))
        masks = np.asarray(masks, dtype=np.int64).reshape(-1)
    if check and (masks >= 128).any():
        raise ValueError("a type mask holds the seven types: at most 127")
    return masks.astype(np.uint8)


@dataclass
class ColourFeatures:
    """The typed side of a known ligand, what `engine.colour` and `engine.combo_overlay` compare a hit's pharmacophore nodes with: `xyz`
    float32 [f, 3] in the pocket's frame, `typemask` uint8 [f] (bit t is type t; 0 pairs with nothing), 1 <= f <= 64; `weights` a dict over
    `constants.DEFAULT_WEIGHTS` (every value finite and >= 0) and `radius` > 0, the one Gaussian radius of every feature and node. Points
    and types only: no donor / acceptor direction, no ring normal."""

    xyz: np.ndarray
    typemask: np.ndarray
    weights: dict = field(default_factory=lambda: dict(DEFAULT_WEIGHTS))
    radius: float = 1.0
    _device: dict = field(default_factory=dict, repr=False, compare=False)  # device index -> the engine's handle, made on first use

    def __len__(self) -> int:
        return len(self.typemask)

    def weights_array(self) -> np.ndarray:
        return np.asarray(weights_vector(self.weights), dtype=np.float32)

    def types(self, i: int) -> list[str]:
        """The type names of feature i."""
        return [name for t, name in enumerate(TYPE_NAMES) if (int(self.typemask[i]) >> t) & 1]

    @classmethod
    def from_arrays(cls, xyz, types, weights: dict | None = None, radius: float = 1.0) -> "ColourFeatures":
        """`types`: per feature a type name, a type id, or - a uint8 array - a mask (`type_masks`)."""
        xyz = np.ascontiguousarray(np.asarray(xyz, dtype=np.float32).reshape(-1, 3))
        masks = np.ascontiguousarray(type_masks(types))
        f = len(xyz)
        if len(masks) != f:
            raise ValueError(f"{len(masks)} types for {f} features")
        if not 1 <= f <= MAX_FEATURES:
            raise ValueError(f"{f} features: a colour reference holds 1 to {MAX_FEATURES}")
        if not np.isfinite(xyz).all():
            raise ValueError("positions must be finite")
        if not (np.isfinite(radius) and radius > 0):
            raise ValueError("radius must be finite and > 0")
        w = dict(DEFAULT_WEIGHTS)
        w.update(weights or {})
        vec = np.asarray(weights_vector(w), dtype=np.float64)
        if not (np.isfinite(vec).all() and (vec >= 0).all()):
            raise ValueError("weights must be finite and not negative")
        return cls(xyz=xyz, typemask=masks, weights=w, radius=float(radius))

    @classmethod
    def from_library(cls, library, index: int, conformer: int = 0, rotation=None, translation=None, weights: dict | None = None, radius: float = 1.0) -> "ColourFeatures":
        """The nodes and type masks of library ligand `index` at `conformer` (`PackedLibrary.unpack`) as the features: a known binder that
        is a record of a library - under `rotation` / `translation` where given, by `ReferenceLigand.from_pose`'s formula."""
        from .library import as_packed_library

        rec = as_packed_library(library).unpack(int(index))
        if not 0 <= int(conformer) < rec["n_conf"]:
            raise ValueError(f"conformer {conformer}: ligand {index} has {rec['n_conf']}")
        xyz = np.ascontiguousarray(rec["xyz"][:, :, int(conformer)])
        if rotation is not None or translation is not None:
            xyz = _posed(xyz, np.eye(3) if rotation is None else rotation, np.zeros(3) if translation is None else translation)
        return cls.from_arrays(xyz, np.asarray(rec["typemask"], dtype=np.uint8), weights, radius)

    @classmethod
    def from_csv(cls, path, weights: dict | None = None, radius: float = 1.0) -> "ColourFeatures":
        """Lines `type,x,y,z`, type a name of `constants.TYPE_NAMES` (a feature of several types: the names joined by `|`); empty lines,
        lines that begin with `#` and a header line `type,x,y,z` are passed over. A name that is no type is refused by name."""
        names, xyz = [], []
        for no, line in enumerate(Path(path).read_text().splitlines(), 1):
            line = line.strip()
            if not line or line.startswith("#") or line.replace(" ", "").lower() == "type,x,y,z":
                continue
            cells = [c.strip() for c in line.split(",")]
            if len(cells) != 4:
                raise ValueError(f"{path}:{no}: expected type,x,y,z")
            for name in cells[0].split("|"):
                if name.strip() not in TYPE_ID:
                    raise ValueError(f"{path}:{no}: {name.strip()!r} is no pharmacophore type: one of {', '.join(TYPE_NAMES)}")
            names.append(cells[0])
            xyz.append([float(c) for c in cells[1:]])
        return cls.from_arrays(np.asarray(xyz, dtype=np.float32).reshape(-1, 3), names, weights, radius)

    def to_csv(self, path) -> None:
        """One line per feature that has a type, `type,x,y,z` with the types joined by `|` and the `repr` of each float32 coordinate:
        `from_csv` reads it back as it is. A feature without a type pairs with nothing and is left out."""
        lines = ["type,x,y,z"]
        for i in range(len(self)):
            if self.typemask[i]:
                lines.append(",".join(["|".join(self.types(i))] + [repr(float(v)) for v in self.xyz[i]]))
        Path(path).write_text("\n".join(lines) + "\n")


@dataclass
class ReferenceLigand:
    """`xyz` float32 [m, 3] in the pocket's frame, `radius` float32 [m]: 1 <= m <= 256, every value finite, every radius > 0."""

    xyz: np.ndarray
    radius: np.ndarray
    _device: dict = field(default_factory=dict, repr=False, compare=False)  # device index -> the engine's handle, made on first use
    colour: "ColourFeatures | None" = None  # the same ligand's typed features, where it has them: what `engine.combo_overlay` adds to the shape

    def __len__(self) -> int:
        return len(self.radius)

    @classmethod
    def from_library(cls, library, index: int, conformer: int = 0, atoms=None, rotation=None, translation=None, node_radius: float = 1.0, weights: dict | None = None,
                     colour_radius: float = 1.0) -> "ReferenceLigand":
        """A known binder that is ligand `index` of a library, atoms and features in one step: the shape side is its heavy atoms at
        `conformer` with Bondi radii from `atoms` (the library's `PackedAtoms`), or without `atoms` its nodes with `node_radius` each; the
        `colour` side is `ColourFeatures.from_library` of the same record. Both under `rotation` / `translation` where given."""
        from .library import as_packed_library

        colour = ColourFeatures.from_library(library, index, conformer, rotation, translation, weights, colour_radius)
        if atoms is None:
            rec = as_packed_library(library).unpack(int(index))
            xyz, radius = np.ascontiguousarray(rec["xyz"][:, :, int(conformer)]), np.full(rec["n_nodes"], node_radius, np.float32)
        else:
            rec = atoms.unpack(int(index))
            if not 0 <= int(conformer) < rec["n_conf"]:
                raise ValueError(f"conformer {conformer}: the atom store has {rec['n_conf']} of ligand {index}")
            xyz, radius = np.ascontiguousarray(rec["xyz"][:, int(conformer), :]), atomic_number_radii(rec["elements"])
        if rotation is not None or translation is not None:
            xyz = _posed(xyz, np.eye(3) if rotation is None else rotation, np.zeros(3) if translation is None else translation)
        out = cls.from_arrays(xyz, radius)
        out.colour = colour
        return out

    @classmethod
    def from_arrays(cls, xyz, radius) -> "ReferenceLigand":
        xyz = np.ascontiguousarray(np.asarray(xyz, dtype=np.float32).reshape(-1, 3))
        radius = np.ascontiguousarray(np.asarray(radius, dtype=np.float32).reshape(-1))
        m = len(xyz)
        if len(radius) != m:
            raise ValueError(f"{len(radius)} radii for {m} atoms")
        if not 1 <= m <= MAX_ATOMS:
            raise ValueError(f"{m} atoms: a reference ligand holds 1 to {MAX_ATOMS}")
        if not np.isfinite(xyz).all():
            raise ValueError("positions must be finite")
        if not (np.isfinite(radius).all() and (radius > 0).all()):
            raise ValueError("radii must be finite and > 0")
        return cls(xyz=xyz, radius=radius)

    @classmethod
    def from_elements(cls, xyz, atomic_numbers) -> "ReferenceLigand":
        """Bondi radii by atomic number (`pocket.atomic_number_radii`): the radii the atom store gives a library's atoms."""
        return cls.from_arrays(xyz, atomic_number_radii(atomic_numbers))

    @classmethod
    def from_pdb(cls, text_or_path, resname: str | None = None) -> "ReferenceLigand":
        """From a PDB text, or the path of a PDB file, through `pocket.parse_pdb_atoms`: the heavy atoms of its ATOM / HETATM records -
        those of residue `resname` alone where that is given - with Bondi radii by element."""
        text = text_or_path
        if isinstance(text_or_path, os.PathLike) or (isinstance(text_or_path, str) and "\n" not in text_or_path and not text_or_path.startswith(("ATOM", "HETATM"))):
            text = Path(text_or_path).read_text()
        atoms = parse_pdb_atoms(str(text))
        if resname is not None:
            atoms = atoms.take(np.array([r == str(resname).strip().upper() for r in atoms.resname], dtype=bool))
        if len(atoms) == 0:
            raise ValueError("no heavy atom" + (f" of residue {resname!r}" if resname is not None else "") + " in the PDB text")
        return cls.from_arrays(atoms.xyz, element_radii(atoms.element))

    @classmethod
    def from_pose(cls, xyz, radius, rotation, translation) -> "ReferenceLigand":
        """Any posed point set as the reference: point x sits at p_k = ((R[k][0] x_0 + R[k][1] x_1) + R[k][2] x_2) + t_k, float64 with every
        operation rounded (the posed point of include/pmx.h), rounded to float32 once."""
        x = np.asarray(xyz, dtype=np.float32).reshape(-1, 3).astype(np.float64)
        R = np.asarray(rotation, dtype=np.float64).reshape(3, 3)
        t = np.asarray(translation, dtype=np.float64).reshape(3)
        p = np.stack([((R[k, 0] * x[:, 0] + R[k, 1] * x[:, 1]) + R[k, 2] * x[:, 2]) + t[k] for k in range(3)], axis=1)
        return cls.from_arrays(p.astype(np.float32), radius)
