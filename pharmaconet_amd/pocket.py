"""The pocket's atoms, for the excluded-volume check of posed hits (`engine.clashes`, `pmx_pose_clash` in include/pmx.h).

A model carries its protein as `PharmacophoreModel.pdbblock` (the reference's `module.py:123-125` puts the file there, joined with an
extra newline per line). `parse_pdb_atoms` reads the heavy atoms out of such a block, `PocketAtoms` is what the device gets: float32
positions in the model's frame, Bondi radii, and per atom the residue it belongs to as one of 256 groups - the bits of a hit's contact
fingerprint. Host code, NumPy only; the device copy is made by `engine` on first use and freed with the object.
"""

from __future__ import annotations

import os
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

__all__ = ["PdbAtoms", "PocketAtoms", "parse_pdb_atoms", "element_radii", "atomic_number_radii", "BONDI", "DEFAULT_RADIUS", "NO_GROUP", "MAX_GROUPS", "MAX_ATOMS"]

# Bondi (1964) van der Waals radii in Angstrom, by element symbol (upper case) and by atomic number; anything else takes DEFAULT_RADIUS
BONDI = {"C": 1.70, "N": 1.55, "O": 1.52, "F": 1.47, "P": 1.80, "S": 1.80, "CL": 1.75, "BR": 1.85, "I": 1.98, "SE": 1.90}
BONDI_Z = {6: 1.70, 7: 1.55, 8: 1.52, 9: 1.47, 15: 1.80, 16: 1.80, 17: 1.75, 35: 1.85, 53: 1.98, 34: 1.90}
DEFAULT_RADIUS = 1.60
NO_GROUP = 0xFFFF  # an atom of none of the 256 residues
MAX_GROUPS = 256  # PMX_MAX_MODEL_NODES: the bits of a fingerprint
MAX_ATOMS = 65536  # PMX_POCKET_MAX_ATOMS
WATER = ("HOH", "WAT", "DOD")
# the two-letter symbols an atom name is read as when the element columns are blank and the name starts in column 13
TWO_LETTER = frozenset("CL BR SE MG ZN FE MN CA NA CU NI CO LI SI AL CD AU AG PT HG AS SR BA CS RB PB".split())


def element_radii(elements) -> np.ndarray:
    """float32 radii of element symbols (any case)."""
    return np.array([BONDI.get(str(e).strip().upper(), DEFAULT_RADIUS) for e in elements], dtype=np.float32)


def atomic_number_radii(numbers) -> np.ndarray:
    """float32 radii of atomic numbers: the same table, for a ligand's atoms."""
    return np.array([BONDI_Z.get(int(z), DEFAULT_RADIUS) for z in np.asarray(numbers).reshape(-1)], dtype=np.float32)


@dataclass
class PdbAtoms:
    """What `parse_pdb_atoms` returns, one entry per kept atom, in file order."""

    xyz: np.ndarray  # float32 [n, 3]
    element: np.ndarray  # str [n], upper case
    name: np.ndarray  # str [n], atom name without blanks
    resname: np.ndarray  # str [n]
    chain: np.ndarray  # str [n]
    resseq: np.ndarray  # int64 [n]
    serial: np.ndarray  # int64 [n]
    icode: np.ndarray  # str [n], insertion code ('' for none)

    def __len__(self) -> int:
        return len(self.serial)

    def take(self, keep) -> "PdbAtoms":
        return PdbAtoms(*(getattr(self, f)[keep] for f in ("xyz", "element", "name", "resname", "chain", "resseq", "serial", "icode")))


def _element_of(line: str) -> str:
    """Columns 77-78, upper-cased; when blank, from the atom name in columns 13-16: two letters when column 13 is a letter and the two
    form a known element (a four-character name that starts with H is a hydrogen: HG11, HE21), otherwise the name's first letter."""
    el = line[76:78].strip().upper()
    if el:
        return el
    name = line[12:16].upper()
    if name[:1].isalpha():
        if name[0] in "HD" and len(name.strip()) == 4:
            return name[0]
        if name[:2] in TWO_LETTER:
            return name[:2]
    for ch in name:
        if ch.isalpha():
            return ch
    return ""


def _int(text: str) -> int:
    try:
        return int(text)
    except ValueError:
        return int(text, 16) if text.strip() else 0  # (serials past 99999 are written in hexadecimal by some programs)


def parse_pdb_atoms(text: str, hetero: bool = True, water: bool = False) -> PdbAtoms:
    """The heavy atoms of the `ATOM` / `HETATM` records of a PDB text, by fixed columns. Empty lines are skipped (the reference's
    `pdbblock` has one after every record); only the first `MODEL` is read; an atom is kept when its altLoc (column 17) is blank or `A`;
    H and D are skipped, the residues HOH / WAT / DOD unless `water`, `HETATM` records unless `hetero`. Coordinates are columns 31-54."""
    rows = []
    for line in text.splitlines():
        rec = line[:6]
        if rec == "ENDMDL":
            break
        if rec not in ("ATOM  ", "HETATM") or len(line) < 54:
            continue
        if rec == "HETATM" and not hetero:
            continue
        if line[16] not in " A":
            continue
        resname = line[17:20].strip()
        if not water and resname in WATER:
            continue
        el = _element_of(line)
        if el in ("H", "D"):
            continue
        rows.append(((line[30:38], line[38:46], line[46:54]), el, line[12:16].strip(), resname, line[21].strip(), _int(line[22:26]), _int(line[6:11]), line[26:27].strip()))
    n = len(rows)
    return PdbAtoms(
        xyz=np.array([[float(v) for v in r[0]] for r in rows], dtype=np.float32).reshape(n, 3),
        element=np.array([r[1] for r in rows], dtype=object),
        name=np.array([r[2] for r in rows], dtype=object),
        resname=np.array([r[3] for r in rows], dtype=object),
        chain=np.array([r[4] for r in rows], dtype=object),
        resseq=np.array([r[5] for r in rows], dtype=np.int64),
        serial=np.array([r[6] for r in rows], dtype=np.int64),
        icode=np.array([r[7] for r in rows], dtype=object),
    )


def _nearest(xyz: np.ndarray, centers: np.ndarray) -> np.ndarray:
    """Per atom the distance to the nearest of `centers` (float64)."""
    if len(xyz) == 0:
        return np.zeros(0)
    d2 = np.full(len(xyz), np.inf)
    x = xyz.astype(np.float64)
    for c in np.asarray(centers, dtype=np.float64).reshape(-1, 3):
        d2 = np.minimum(d2, ((x - c) ** 2).sum(axis=1))
    return np.sqrt(d2)


def residue_groups(atoms: PdbAtoms, centers=None) -> tuple[np.ndarray, list[str]]:
    """(group uint16 [n], labels): a residue is (chain, number, insertion code, name). With `centers` the 256 residues whose nearest atom lies
    closest to any of them get the ids 0 .. 255 in that order, ties in file order; without, the first 256 residues of the file. Every other
    atom gets 0xFFFF. A label reads `A:CYS12` (`A:CYS12B` with an insertion code)."""
    keys: dict[tuple, int] = {}
    res_of = np.zeros(len(atoms), dtype=np.int64)
    for i in range(len(atoms)):
        k = (atoms.chain[i], int(atoms.resseq[i]), atoms.icode[i], atoms.resname[i])
        res_of[i] = keys.setdefault(k, len(keys))
    order = np.arange(len(keys))
    if centers is not None and len(np.asarray(centers).reshape(-1, 3)) and len(keys):
        near = np.full(len(keys), np.inf)
        np.minimum.at(near, res_of, _nearest(atoms.xyz, centers))
        order = np.argsort(near, kind="stable")
    order = order[:MAX_GROUPS]
    gid = np.full(len(keys), NO_GROUP, dtype=np.uint16)
    gid[order] = np.arange(len(order), dtype=np.uint16)
    names = list(keys)
    labels = [f"{names[r][0]}:{names[r][3]}{names[r][1]}{names[r][2]}" for r in order]
    return (gid[res_of] if len(atoms) else np.zeros(0, np.uint16)), labels


@dataclass
class PocketAtoms:
    """The atoms a posed hit is checked against: `xyz` float32 [n, 3] in the model's frame, `radius` float32 [n], `group` uint16 [n] (the
    residue's bit of a contact fingerprint, 0xFFFF for none), `residue_labels` naming the groups, `atom_labels` naming the atoms
    (`A:CYS12:SG`; None for a pocket made from arrays)."""

    xyz: np.ndarray
    radius: np.ndarray
    group: np.ndarray
    residue_labels: list = field(default_factory=list)
    atom_labels: "list | None" = None
    _device: dict = field(default_factory=dict, repr=False, compare=False)  # device index -> the engine's handle, made on first use

    def __len__(self) -> int:
        return len(self.radius)

    @classmethod
    def from_arrays(cls, xyz, radius, group=None) -> "PocketAtoms":
        xyz = np.ascontiguousarray(np.asarray(xyz, dtype=np.float32).reshape(-1, 3))
        radius = np.ascontiguousarray(np.asarray(radius, dtype=np.float32).reshape(-1))
        n = len(xyz)
        if len(radius) != n:
            raise ValueError(f"{len(radius)} radii for {n} atoms")
        group = np.full(n, NO_GROUP, dtype=np.uint16) if group is None else np.ascontiguousarray(np.asarray(group, dtype=np.uint16).reshape(-1))
        if len(group) != n:
            raise ValueError(f"{len(group)} groups for {n} atoms")
        if n > MAX_ATOMS:
            raise ValueError(f"{n} atoms: a pocket holds at most {MAX_ATOMS} (cut it with `within`)")
        if not (np.isfinite(xyz).all() and np.isfinite(radius).all()):
            raise ValueError("positions and radii must be finite")
        used = sorted({int(g) for g in group if g < MAX_GROUPS})
        return cls(xyz=xyz, radius=radius, group=group, residue_labels=[f"group{g}" for g in range(used[-1] + 1)] if used else [])

    @classmethod
    def from_pdb(cls, text_or_path, centers=None, within: float | None = None, hetero: bool = True, water: bool = False) -> "PocketAtoms":
        """From a PDB text, or the path of a PDB file. `within` keeps the atoms within that many Angstrom of any of `centers`; the default
        keeps everything (a protein is a few thousand atoms, and a posed ligand can reach well outside the hotspots)."""
        text = text_or_path
        if isinstance(text_or_path, os.PathLike) or (isinstance(text_or_path, str) and "\n" not in text_or_path and not text_or_path.startswith(("ATOM", "HETATM"))):
            text = Path(text_or_path).read_text()
        atoms = parse_pdb_atoms(str(text), hetero=hetero, water=water)
        if within is not None:
            if centers is None:
                raise ValueError("`within` needs `centers`")
            atoms = atoms.take(_nearest(atoms.xyz, centers) <= float(within))
        group, labels = residue_groups(atoms, centers)
        out = cls.from_arrays(atoms.xyz, element_radii(atoms.element), group)
        out.residue_labels = labels
        out.atom_labels = [f"{atoms.chain[i]}:{atoms.resname[i]}{int(atoms.resseq[i])}{atoms.icode[i]}:{atoms.name[i]}" for i in range(len(atoms))]
        return out

    @classmethod
    def from_model(cls, model, within: float | None = None, hetero: bool = True, water: bool = False) -> "PocketAtoms":
        """From the protein a model carries (`PharmacophoreModel.pdbblock`), grouped around the model's node centres."""
        block = model.pdbblock
        if not block or not any(ln.startswith(("ATOM  ", "HETATM")) for ln in str(block).splitlines()):
            raise ValueError(f"the model's pdbblock holds no ATOM / HETATM record ({str(block)[:40]!r}): give the protein with PocketAtoms.from_pdb")
        return cls.from_pdb(str(block) if "\n" in str(block) else str(block) + "\n", centers=model.node_centers, within=within, hetero=hetero, water=water)

    def residues(self, fingerprint) -> list[str]:
        """The labels of the groups whose bits are set in a uint64 [4] contact fingerprint, in group order."""
        bits = np.unpackbits(np.ascontiguousarray(np.asarray(fingerprint, dtype=np.uint64).reshape(-1)).view(np.uint8), bitorder="little")
        return [self.residue_labels[g] if g < len(self.residue_labels) else f"group{g}" for g in np.flatnonzero(bits)]

    def atom_label(self, index: int) -> str:
        if index < 0:
            return ""
        return self.atom_labels[index] if self.atom_labels is not None else f"atom{int(index)}"
