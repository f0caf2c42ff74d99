"""NumPy restatement of the atom store (`pmx_atoms` in include/pmx.h): the record, written byte by byte with `struct`, and the gather of
`pmx_atoms_gather`, one row at a time. Nothing here shares code with pharmaconet_amd/atoms.py.

Record: u16 n_atoms | u16 n_conf | u32 0 | u8 element[n_atoms] | pad to 4 | f32 xyz[n_atoms][n_conf][3] | pad to 16. Header-only (16 zero
bytes but for nothing: n_atoms = 0, n_conf = 0) for a molecule with no heavy atom, more than 256, no conformer or more than 64, or one
flagged as unsupported."""

import struct

import numpy as np

OK, UNSUPPORTED, KEY_INVALID = 0, 1, 4
MAX_ATOMS, MAX_CONF = 256, 64


def record(z, positions, supported=True) -> bytes:
    """The record of one molecule: `z` atomic numbers of all atoms, `positions` float32 [n, C, 3]."""
    z = np.asarray(z, dtype=np.int64).reshape(-1)
    pos = np.asarray(positions, dtype=np.float32)
    heavy = np.flatnonzero(z > 1)
    C = pos.shape[1] if pos.ndim == 3 else 0
    if not supported or not 1 <= len(heavy) <= MAX_ATOMS or not 1 <= C <= MAX_CONF:
        return struct.pack("<HHI", 0, 0, 0) + b"\0" * 8
    out = bytearray(struct.pack("<HHI", len(heavy), C, 0))
    for a in heavy:
        if z[a] > 127:
            raise ValueError("element above 127")
        out += struct.pack("<B", int(z[a]))
    out += b"\0" * (-len(out) % 4)
    for a in heavy:
        for c in range(C):
            out += struct.pack("<3f", *(float(v) for v in pos[a, c]))
    out += b"\0" * (-len(out) % 16)
    return bytes(out)


def store(zs, positions, supported=None):
    """(offsets u64 [N + 1], data u8) of a list of molecules."""
    recs = [record(z, p, True if supported is None else bool(supported[i])) for i, (z, p) in enumerate(zip(zs, positions))]
    offsets = np.zeros(len(recs) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in recs])
    return offsets, np.frombuffer(b"".join(recs), dtype=np.uint8).copy()


def parse(offsets, data, i):
    """(elements u8 [n], xyz float32 [n, C, 3]) of record i."""
    base = int(offsets[i])
    n, C, zero = struct.unpack_from("<HHI", data, base)
    assert zero == 0
    at = base + ((8 + n + 3) & ~3)
    return data[base + 8 : base + 8 + n].copy(), np.frombuffer(data[at : at + 12 * n * C].tobytes(), dtype="<f4").reshape(n, C, 3)


def gather(offsets, data, table, ligands, conformers):
    """`pmx_atoms_gather`: (point_off int64 [n + 1], points float32 [total, 3], radii float32 [total], status int32 [n])."""
    N = len(offsets) - 1
    off, pts, rad, status = [0], [], [], []
    for lig, c in zip(ligands, conformers):
        lig, c = int(lig), int(c)
        st, p, r = UNSUPPORTED, np.zeros((0, 3), np.float32), np.zeros(0, np.float32)
        if 0 <= lig < N:
            el, xyz = parse(offsets, data, lig)
            if len(el) > 0:
                if 0 <= c < xyz.shape[1]:
                    st, p, r = OK, xyz[:, c], np.asarray(table, dtype=np.float32)[el]
                else:
                    st = KEY_INVALID
        status.append(st)
        pts.append(p)
        rad.append(r)
        off.append(off[-1] + len(p))
    return (np.array(off, np.int64), np.concatenate(pts + [np.zeros((0, 3), np.float32)]).astype(np.float32), np.concatenate(rad + [np.zeros(0, np.float32)]).astype(np.float32),
            np.array(status, np.int32))
