"""The atom store: each ligand's heavy atoms next to its packed record (`pmx_atoms` in include/pmx.h, csrc/pmx_atoms.hip).

A `PackedAtoms` is the companion of a `PackedLibrary`: one record per ligand, in the library's order, holding the atomic numbers and the
float32 positions of the molecule's heavy atoms (Z > 1) at every conformer, in the frame the packed record's nodes are in. Uploaded
(`engine.DeviceAtoms`) it feeds the point-mode rows of `clashes`, `refine` and the atom-level `pose_search` on the device.

Record (little endian, padded to 16 bytes):
    u16 n_atoms | u16 n_conf | u32 0
    u8  element[n_atoms]
    pad to 4 bytes
    f32 xyz[n_atoms][n_conf][3]     == atom_positions[heavy] as it lies in `LigandFeatures`
A header-only record (16 bytes, n_atoms = 0) means "no atoms kept": a molecule with more than `MAX_LIGAND_ATOMS` heavy atoms, with none,
with no or more than 64 conformers, or whose packed record is `UNSUPPORTED_RECORD`."""

from __future__ import annotations

import struct
from dataclasses import dataclass
from pathlib import Path
from typing import Sequence

import numpy as np

from .library import RECORD_ALIGN, PackedLibrary

MAX_LIGAND_ATOMS = 256  # include/pmx.h PMX_MAX_LIGAND_ATOMS
MAX_CONFORMERS = 64  # PMX_MAX_CONFORMERS
MAX_ELEMENT = 127
_HEADER = struct.Struct("<HHI")
_MAGIC = b"PMXATM01"
HEADER_ONLY = _HEADER.pack(0, 0, 0) + b"\0" * (RECORD_ALIGN - _HEADER.size)


def _xyz_at(n):
    """Where a record of n atoms keeps its coordinates (bytes from its start)."""
    return (_HEADER.size + n + 3) & ~3


def supported_mask(library: PackedLibrary) -> np.ndarray:
    """bool [N]: the ligands of `library` whose record is not `UNSUPPORTED_RECORD`, the all-zero header."""
    return library.headers().any(axis=1)


def _atomic_numbers(mol) -> np.ndarray:
    z = getattr(mol, "atomic_nums", None)
    if z is None:
        z = mol.answers["atomic_num"]  # a `ligand.Ligand`: its toolkit answers
    return np.asarray(z, dtype=np.int64).reshape(-1)


@dataclass
class PackedAtoms:
    offsets: np.ndarray  # u64 [N + 1]
    data: np.ndarray  # u8 [offsets[-1]]

    def __len__(self) -> int:
        return int(self.offsets.shape[0]) - 1

    # -- construction ----------------------------------------------------------
    @classmethod
    def from_flat(cls, flat: dict, supported=None) -> "PackedAtoms":
        """From the flat feature batch of `library.flatten_features` (its `atom_off`, `atomic_num`, `n_conf`, `pos_off` and `positions`): a
        masked copy, no loop over atoms. `supported`: bool [N], False where the ligand's packed record is the unsupported marker
        (`supported_mask(library)`, or the packer's status == 0); None keeps every molecule within the store's own limits."""
        atom_off = np.asarray(flat["atom_off"]).astype(np.int64)
        z = np.asarray(flat["atomic_num"]).astype(np.int64).reshape(-1)
        n_conf = np.asarray(flat["n_conf"]).astype(np.int64).reshape(-1)
        pos_off = np.asarray(flat["pos_off"]).astype(np.int64)
        positions = np.ascontiguousarray(flat["positions"], dtype=np.float32).reshape(-1)
        N = len(atom_off) - 1
        if len(n_conf) != N or len(pos_off) != N + 1 or (N and int(atom_off[-1]) != len(z)):
            raise ValueError("PackedAtoms: atom_off, n_conf and pos_off do not describe one batch")
        if z.size and int(z.max()) > MAX_ELEMENT:
            bad = int(np.flatnonzero(z > MAX_ELEMENT)[0])
            raise ValueError(f"PackedAtoms: atomic number {int(z[bad])} above {MAX_ELEMENT} (atom {bad} of the batch)")
        heavy = z > 1
        before = np.concatenate([[0], np.cumsum(heavy)]).astype(np.int64)  # heavy atoms before atom g of the batch
        na = np.diff(atom_off)
        nh = before[atom_off[1:]] - before[atom_off[:-1]]
        keep = (nh >= 1) & (nh <= MAX_LIGAND_ATOMS) & (n_conf >= 1) & (n_conf <= MAX_CONFORMERS) & (np.diff(pos_off) == na * n_conf * 3)
        if supported is not None:
            supported = np.asarray(supported, dtype=bool).reshape(-1)
            if len(supported) != N:
                raise ValueError(f"PackedAtoms: {len(supported)} flags for {N} molecules")
            keep &= supported
        n_rec, c_rec = np.where(keep, nh, 0), np.where(keep, n_conf, 0)
        sizes = np.where(keep, (_xyz_at(n_rec) + 12 * n_rec * c_rec + RECORD_ALIGN - 1) // RECORD_ALIGN * RECORD_ALIGN, RECORD_ALIGN)
        offsets = np.zeros(N + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum(sizes)
        data = np.zeros(int(offsets[-1]), dtype=np.uint8)
        start = offsets[:-1].astype(np.int64)
        head = data.view("<u2")  # (records start on 16 bytes)
        head[start // 2] = n_rec.astype(np.uint16)
        head[start // 2 + 1] = c_rec.astype(np.uint16)
        # the heavy atoms of the kept molecules, in batch order
        mol_of = np.repeat(np.arange(N, dtype=np.int64), na)
        g = np.flatnonzero(heavy & keep[mol_of])
        if g.size:
            m = mol_of[g]
            rank = before[g] - before[atom_off[m]]  # the atom's place among its molecule's heavy atoms
            data[start[m] + _HEADER.size + rank] = z[g].astype(np.uint8)
            run = 3 * n_conf[m]  # floats per atom
            ends = np.cumsum(run)
            ramp = np.arange(int(ends[-1]), dtype=np.int64) - np.repeat(ends - run, run)
            src = np.repeat(pos_off[m] + (g - atom_off[m]) * run, run) + ramp
            dst = np.repeat((start[m] + _xyz_at(n_rec[m])) // 4 + rank * run, run) + ramp
            data.view("<f4")[dst] = positions[src]
        return cls(offsets, data)

    @classmethod
    def from_arrays(cls, elements: Sequence, positions: Sequence, supported=None) -> "PackedAtoms":
        """From per-ligand arrays: `elements[i]` the atomic numbers of all atoms [n_i], `positions[i]` float32 [n_i, C_i, 3]. Hydrogens
        are left out here as everywhere."""
        if len(elements) != len(positions):
            raise ValueError(f"{len(elements)} element lists for {len(positions)} position arrays")
        zs = [np.asarray(e, dtype=np.int64).reshape(-1) for e in elements]
        for e in zs:
            if e.size and (int(e.max()) > MAX_ELEMENT or int(e.min()) < 0):
                raise ValueError(f"PackedAtoms: atomic number outside 0 .. {MAX_ELEMENT}")
        ps = []
        for e, p in zip(zs, positions):
            p = np.ascontiguousarray(p, dtype=np.float32)
            if p.ndim != 3 or p.shape[0] != len(e) or p.shape[2] != 3:
                p = p.reshape(len(e), -1, 3) if len(e) and p.size and p.size % (3 * len(e)) == 0 else np.zeros((len(e), 0, 3), np.float32)
            ps.append(p)
        atom_off = np.concatenate([[0], np.cumsum([len(e) for e in zs])]).astype(np.int64)
        pos_off = np.concatenate([[0], np.cumsum([p.size for p in ps])]).astype(np.int64)
        flat = dict(atom_off=atom_off, atomic_num=np.concatenate(zs + [np.zeros(0, np.int64)]), n_conf=np.array([p.shape[1] for p in ps], np.int64), pos_off=pos_off,
                    positions=np.concatenate([p.reshape(-1) for p in ps] + [np.zeros(0, np.float32)]))
        return cls.from_flat(flat, supported)

    @classmethod
    def from_features(cls, mols: Sequence, supported=None) -> "PackedAtoms":
        """From `LigandFeatures` / `Ligand` objects, the molecules a library was packed from, in its order."""
        return cls.from_arrays([_atomic_numbers(m) for m in mols], [np.asarray(m.atom_positions, dtype=np.float32) for m in mols], supported)

    @classmethod
    def for_library(cls, mols, library: PackedLibrary) -> "PackedAtoms":
        """`from_features` (or `from_flat`, for a flat batch) as the companion of `library`: its unsupported records get no atoms."""
        if len(library) != (len(mols["atom_off"]) - 1 if isinstance(mols, dict) else len(mols)):
            raise ValueError("PackedAtoms.for_library: the molecules are not the library's")
        mask = supported_mask(library)
        return cls.from_flat(mols, mask) if isinstance(mols, dict) else cls.from_features(mols, mask)

    # -- reading ---------------------------------------------------------------
    def headers(self) -> np.ndarray:
        """int64 [N, 2]: n_atoms, n_conf."""
        start = self.offsets[:-1].astype(np.int64) // 2
        head = np.ascontiguousarray(self.data).view("<u2")
        return np.stack([head[start], head[start + 1]], axis=1).astype(np.int64) if len(self) else np.zeros((0, 2), np.int64)

    @property
    def max_atoms(self) -> int:
        return int(self.headers()[:, 0].max()) if len(self) else 0

    def record(self, i: int) -> bytes:
        return self.data[int(self.offsets[i]) : int(self.offsets[i + 1])].tobytes()

    def unpack(self, i: int) -> dict:
        """Record i: n_atoms, n_conf, elements u8 [n_atoms], xyz float32 [n_atoms, n_conf, 3]."""
        base = int(self.offsets[i])
        n, c, _ = _HEADER.unpack_from(self.data, base)
        at = base + _xyz_at(n)
        return dict(n_atoms=n, n_conf=c, elements=self.data[base + _HEADER.size : base + _HEADER.size + n].copy(),
                    xyz=self.data[at : at + 12 * n * c].view("<f4").reshape(n, c, 3).copy())

    def _as_library(self) -> PackedLibrary:
        return PackedLibrary(self.offsets, self.data)  # (the record arithmetic of `select` and `slice` is the same: 16-byte units)

    def slice(self, first: int, count: int) -> "PackedAtoms":
        part = self._as_library().slice(first, count)
        return PackedAtoms(part.offsets, part.data)

    def select(self, indices) -> "PackedAtoms":
        """The records of ligands `indices` (any order, repeats allowed): the companion of `PackedLibrary.select(indices)`."""
        part = self._as_library().select(indices)
        return PackedAtoms(part.offsets, part.data)

    # -- storage ---------------------------------------------------------------
    def save(self, path: str | Path) -> None:
        with open(path, "wb") as w:
            w.write(_MAGIC)
            w.write(struct.pack("<QQ", len(self), int(self.data.shape[0])))
            w.write(np.ascontiguousarray(self.offsets, dtype="<u8").tobytes())
            w.write(np.ascontiguousarray(self.data).tobytes())

    @classmethod
    def load(cls, path: str | Path) -> "PackedAtoms":
        with open(path, "rb") as f:
            if f.read(8) != _MAGIC:
                raise ValueError(f"{path}: not an atom store")
            n, nbytes = struct.unpack("<QQ", f.read(16))
            offsets = np.frombuffer(f.read(8 * (n + 1)), dtype="<u8").astype(np.uint64)
            data = np.frombuffer(f.read(nbytes), dtype=np.uint8).copy()
        if offsets.shape[0] != n + 1 or data.shape[0] != nbytes or int(offsets[-1]) != nbytes:
            raise ValueError(f"{path}: truncated atom store")
        return cls(offsets, data)


def atoms_path(library_path: str | Path) -> Path:
    """Where the store of a saved library lies: `X.pmxlib` -> `X.pmxlib.atoms`."""
    return Path(str(library_path) + ".atoms")
