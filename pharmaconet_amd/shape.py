"""The reference ligand posed hits are compared with: the known binder of a structure-based screen, as atoms in the pocket's frame.

`ReferenceLigand` is what `engine.shape` takes - positions and radii, made from arrays, from atomic numbers, from a PDB file, or from any
posed set of points (a hit's own fitted pose, to compare the other hits with). The overlap itself is `pmx_pose_shape` (include/pmx.h).
"""

from __future__ import annotations

import os
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

from .pocket import atomic_number_radii, element_radii, parse_pdb_atoms

MAX_ATOMS = 256  # PMX_MAX_LIGAND_ATOMS


@dataclass
class ReferenceLigand:
    """`xyz` float32 [m, 3] in the pocket's frame, `radius` float32 [m]: 1 <= m <= 256, every value finite, every radius > 0."""

    xyz: np.ndarray
    radius: np.ndarray
    _device: dict = field(default_factory=dict, repr=False, compare=False)  # device index -> the engine's handle, made on first use

    def __len__(self) -> int:
        return len(self.radius)

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
