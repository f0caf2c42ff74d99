#!/usr/bin/env python3
"""Mint the clash fixtures from the reference's example structure. Build container only (needs the reference's `examples/`):

    python tests/golden/make_golden_pocket_6oim.py [REFERENCE_DIR]

Written next to this file, data only (PDB records copied line by line, nothing of the reference's programs):
  pocket_6oim.pdb      every ATOM / HETATM line of examples/6OIM_protein.pdb whose atom lies within 12 A of a heavy atom of
                       examples/6OIM_D_MOV.pdb - hydrogens and waters stay in, so that the reader's filters have something to drop
  ligand_6oim_mov.pdb  the HETATM lines of examples/6OIM_D_MOV.pdb (the crystal ligand, 41 heavy atoms)
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
WITHIN = 12.0


def records(path: Path) -> list[str]:
    return [ln.rstrip("\n") for ln in path.read_text().splitlines() if ln.startswith(("ATOM  ", "HETATM"))]


def xyz(lines: list[str]) -> np.ndarray:
    return np.array([[float(ln[30:38]), float(ln[38:46]), float(ln[46:54])] for ln in lines], dtype=np.float64).reshape(-1, 3)


def element(ln: str) -> str:
    return ln[76:78].strip().upper()


def main() -> None:
    ref = Path(sys.argv[1]) if len(sys.argv) > 1 else Path("/root/reference")
    protein = records(ref / "examples" / "6OIM_protein.pdb")
    ligand = records(ref / "examples" / "6OIM_D_MOV.pdb")
    heavy = xyz([ln for ln in ligand if element(ln) not in ("H", "D")])
    p = xyz(protein)
    d2 = ((p[:, None, :] - heavy[None, :, :]) ** 2).sum(-1).min(axis=1)
    keep = [ln for ln, v in zip(protein, d2) if v <= WITHIN * WITHIN]
    (HERE / "pocket_6oim.pdb").write_text("".join(ln + "\n" for ln in keep))
    (HERE / "ligand_6oim_mov.pdb").write_text("".join(ln + "\n" for ln in ligand))
    print(f"pocket_6oim.pdb: {len(keep)} of {len(protein)} records; ligand_6oim_mov.pdb: {len(ligand)} records")


if __name__ == "__main__":
    main()
