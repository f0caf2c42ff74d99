"""The posed-hit layer: rows of points under a rigid motion, judged against the pocket (`clashes`, `refine`), a known ligand (`shape`,
`overlay`, and with its typed features `colour`, `combo_overlay`) or the model's hotspots (`pose_fit`). `engine.py` re-exports every name of this module."""

from __future__ import annotations

import contextlib
import ctypes
from dataclasses import dataclass

import numpy as np

from . import _ffi
from ._device import (_FP_WORDS, _MAX_LEADERS, _MAX_MODEL_NODES, _MAX_NODES, DeviceAtoms, _cached_handle, _device_index, _DeviceHandle, _is_store, _record_counts, _resident,
                      _resident_atoms, _torch, _weights_array, device_model)
from .constants import weights_vector


def _fingerprint_tensor(fp, tdev):
    torch = _torch()
    fp = np.ascontiguousarray(np.asarray(fp, dtype=np.uint64).reshape(-1, _FP_WORDS))
    if len(fp) > 65536:
        raise ValueError("at most 65536 fingerprints per call (PMX_EXPLAIN_MAX)")
    return torch.from_numpy(np.ascontiguousarray(fp.view(np.int64).reshape(max(len(fp), 0), _FP_WORDS))).to(tdev), len(fp)


def fingerprint_similarity(a, b=None, device=None) -> np.ndarray:
    """Tanimoto similarity (`pmx_fingerprint_tanimoto`, csrc/pmx_fingerprint.hip) of the uint64 [n, 4] fingerprints `a` against `b` (default:
    `a` itself): float32 [n, m], popcount(x & y) / popcount(x | y) and 1 where both are empty. Waits for the stream."""
    torch = _torch()
    lib = _ffi.load()
    dev = _device_index(device)
    tdev = torch.device("cuda", dev)
    with torch.cuda.device(tdev):
        ta, na = _fingerprint_tensor(a, tdev)
        tb, nb = (ta, na) if b is None else _fingerprint_tensor(b, tdev)
        out = torch.empty((na, nb), dtype=torch.float32, device=tdev)
        stream = torch.cuda.current_stream(tdev)
        _ffi.check(lib.pmx_fingerprint_tanimoto(ta.data_ptr(), na, tb.data_ptr(), nb, out.data_ptr(), dev, ctypes.c_void_p(stream.cuda_stream)))
        stream.synchronize()
    return out.cpu().numpy()


def fingerprint_leaders(fp, threshold: float = 0.7, max_leaders: int = _MAX_LEADERS, device=None):
    """Sphere exclusion in row order (`pmx_fingerprint_leaders`): (leaders, leader_of) - the rows that became leaders, ascending, and per row
    the leader it joined (itself for a leader; -1 for a row that joined none after `max_leaders` leaders existed). A row joins the first
    earlier leader it is at least `threshold` similar to. Waits for the stream."""
    torch = _torch()
    lib = _ffi.load()
    dev = _device_index(device)
    tdev = torch.device("cuda", dev)
    with torch.cuda.device(tdev):
        t, n = _fingerprint_tensor(fp, tdev)
        leader_of = torch.empty(max(n, 1), dtype=torch.int32, device=tdev)
        leaders = torch.empty(max(int(max_leaders), 1), dtype=torch.int32, device=tdev)
        count = torch.zeros(1, dtype=torch.int32, device=tdev)
        stream = torch.cuda.current_stream(tdev)
        _ffi.check(lib.pmx_fingerprint_leaders(t.data_ptr(), n, float(threshold), int(max_leaders), leader_of.data_ptr(), leaders.data_ptr(), count.data_ptr(), dev,
                                               ctypes.c_void_p(stream.cuda_stream)))
        stream.synchronize()
    nl = int(count.cpu()[0])
    lo = leader_of.cpu().numpy()[:n].view(np.uint32).astype(np.int64)
    lo[lo == 0xFFFFFFFF] = -1
    return leaders.cpu().numpy()[:nl].view(np.uint32).astype(np.int64), lo


class _PosedRows:
    """What every result that holds posed rows can do with them - `Alignment`, `RefinedPoses`, `ShapeOverlay`: row i of what a method returns
    is row i of the poses, and a row that is not OK passes through with status 4. The rows' points are their own pharmacophore nodes with
    `library` alone (node mode: nothing but the resident records is read), the molecules' heavy atoms with Bondi radii with `atoms` - per
    row the `LigandFeatures` / `Ligand` the record was packed from (point mode), or the library's atom store. Written in terms of
    `rotation`, `translation`, `indices` and `conformers`; a message names the class."""

    def _what(self, method: str) -> str:
        return f"{type(self).__name__}.{method}"

    def _library_rows(self, method: str) -> None:
        if self.indices is None:
            raise ValueError(f"{self._what(method)}: these rows are points of the caller's, not ligands of a library")

    def transform(self, i: int, positions) -> np.ndarray:
        """Row i's motion applied to any [..., 3] array of points of the conformer's frame - a whole molecule's atoms, say: positions @ R.T + t."""
        return np.asarray(positions, dtype=np.float64) @ self.rotation[i].T + self.translation[i]

    def clashes(self, pocket_or_model, library=None, atoms=None, **kw) -> "ClashReport":
        """These poses checked against the pocket's atoms (`clashes`). `pocket_or_model`: a `pocket.PocketAtoms`, or a model that carries
        its protein (`PharmacophoreModel.pocket_atoms`). Further arguments as `clashes` takes them."""
        pocket, source = _pose_source(self, self._what("clashes"), pocket_or_model, library, atoms)
        return clashes(pocket, rotation=self.rotation, translation=self.translation, **source, **kw)

    def pose_fit(self, model, library, keys=None, **kw) -> "PoseFit":
        """How well these poses sit on the model's hotspots (`pose_fit`; rows that are ligands of a library only). `keys`: the rows' keys,
        for the pairs the fit was made on (key mode); None for every pair of matching type (free mode). Further arguments (`weights`,
        `centers`, `sigmas`) as `pose_fit` takes them."""
        self._library_rows("pose_fit")
        return pose_fit(model, library, self.indices, self.conformers, self.rotation, self.translation, keys=keys, **kw)

    def shape(self, reference, library=None, atoms=None, **kw) -> "ShapeReport":
        """These poses compared with a known ligand (`shape`; `reference` a `shape.ReferenceLigand`). Further arguments (`node_radius`,
        `cover`) as `shape` takes them."""
        _, source = _pose_source(self, self._what("shape"), None, library, atoms)
        return shape(reference, rotation=self.rotation, translation=self.translation, **source, **kw)


class _Refinable:
    def refine(self, pocket_or_model, library=None, atoms=None, **kw) -> "RefinedPoses":
        """These poses moved out of the pocket's atoms and held near where they are (`refine`; rows that are ligands of a library only): the
        points and the anchors are the rows' nodes, or with `atoms` their heavy atoms. Further arguments (`restraint`, `max_iter`, `ftol`,
        `tolerance`, `node_radius`) as `refine` takes them."""
        self._library_rows("refine")
        pocket, source = _pose_source(self, self._what("refine"), pocket_or_model, library, atoms)
        out = refine(pocket, rotation=self.rotation, translation=self.translation, **source, **kw)
        if out.indices is None:
            out.indices, out.conformers = self.indices.copy(), np.asarray(self.conformers, dtype=np.int64).copy()
        return out


class _Overlayable:
    def overlay(self, reference, library=None, atoms=None, **kw) -> "ShapeOverlay":
        """These poses moved to their nearest shape match with a known ligand (`overlay` from each row's own motion): how far is the pose
        from it, and how much overlap does it lack? Further arguments (`node_radius`, `ftol`, `max_iter`) as `overlay` takes them."""
        what = self._what("overlay")
        if kw.get("starts", 0):
            raise ValueError(f"{what}: the local overlay of these poses; `overlay(..., starts=4)` is the one that needs no pose")
        _, source = _pose_source(self, what, None, library, atoms)
        out = overlay(reference, rotation=self.rotation, translation=self.translation, **source, **kw)
        if out.indices is None and self.indices is not None:
            out.indices, out.conformers = np.asarray(self.indices).copy(), np.asarray(self.conformers, dtype=np.int64).copy()
        return out


@dataclass
class Alignment(_PosedRows, _Refinable, _Overlayable):
    """What `align` returns: one row per (ligand, conformer, key) - the rigid motion that puts the matched nodes of the conformer onto the
    pharmacophore points of the model nodes they are matched to, and how well (definitions: `pmx_align` in include/pmx.h). All float64.

    rotation[i]     [3, 3] proper rotation R        translation[i]  [3] t: a point x of the conformer sits at R x + t in the pocket
    weight[i]       W, the sum of the pair weights  sse[i]          sum over pairs of w |R x_u + t - y_m|^2
    rmsd[i]         sqrt(sse / W)                   rmsd_nodes[i]   the same with every node's targets replaced by their weighted centroid
    scale[i]        E0 = sum w (|x_u - xbar|^2 + |y_m - ybar|^2)
    gap[i]          lambda_1 - lambda_2 of Horn's matrix: where gap / scale is tiny (one fitted node, nodes on a line) the rotation is not unique
    node[i]         [n]: per node of the packed record its distance from its targets' centroid after the fit, -1 for a node without a pair
    n_nodes[i], n_pairs[i]  fitted nodes and pairs  levels[i]       int [nl]: the ligand cluster behind each tree level
    status[i]       0, 1 (PMX_LIGAND_UNSUPPORTED) or 4 (PMX_LIGAND_KEY_INVALID: not a conformer of the ligand, or a match that is no candidate
                    of its level); every float of such a row is NaN. A valid row without pairs has R = I, t = 0 and zeros.
    `transform`, `clashes`, `refine`, `pose_fit`, `shape` and `overlay` of these poses: see `_PosedRows`."""

    indices: np.ndarray
    conformers: np.ndarray
    rotation: np.ndarray
    translation: np.ndarray
    rmsd: np.ndarray
    rmsd_nodes: np.ndarray
    weight: np.ndarray
    sse: np.ndarray
    scale: np.ndarray
    gap: np.ndarray
    node: list
    n_nodes: np.ndarray
    n_pairs: np.ndarray
    levels: list
    status: np.ndarray
    rows: "np.ndarray | None" = None  # `Explanation.poses`: the explanation's row behind each row

    def __len__(self) -> int:
        return len(self.indices)


def _atomic_numbers(mol) -> np.ndarray:
    """Atomic numbers of a `LigandFeatures` (`atomic_nums`) or a `Ligand` (its toolkit answers)."""
    z = getattr(mol, "atomic_nums", None)
    if z is None:
        z = mol.answers["atomic_num"]
    return np.asarray(z, dtype=np.int64).reshape(-1)


@dataclass
class ClashReport:
    """What `clashes` returns: one row per posed set of points (definitions: `pmx_pose_clash` in include/pmx.h).

    clearance[i]    float64: the largest penetration over all (point, atom) pairs - negative when nothing clashes, -inf without a pair
    overlap[i]      float64: the sum of penetration^2 over the clashing pairs
    n_points[i], n_clashing[i], n_pairs[i], n_contacts[i]   points, points with a clashing pair, clashing pairs, points that touch an atom
    worst[i]        (point, atom) of clearance[i]; (-1, -1) without a pair
    point_penetration[i], point_atom[i]   per point its largest penetration and the atom that attains it
    contact_fingerprint   uint64 [n, 4]: bit g says an atom of residue group g touches the row (`PocketAtoms.residue_labels[g]`)
    status[i]       0, 1 (PMX_LIGAND_UNSUPPORTED) or 4 (PMX_LIGAND_KEY_INVALID: not a conformer of the ligand, or a motion that is not
                    finite - a row of an `Alignment` that was not OK); such a row has NaN, zero counts and an empty fingerprint"""

    clearance: np.ndarray
    overlap: np.ndarray
    n_points: np.ndarray
    n_clashing: np.ndarray
    n_pairs: np.ndarray
    n_contacts: np.ndarray
    worst: np.ndarray
    point_penetration: list
    point_atom: list
    contact_fingerprint: np.ndarray
    status: np.ndarray
    device: "int | None" = None  # where `similarity` and `leaders` run

    def __len__(self) -> int:
        return len(self.status)

    def ok(self, max_clashing: int = 0) -> np.ndarray:
        """bool [n]: status 0 and at most `max_clashing` points with a clashing pair."""
        return (self.status == 0) & (self.n_clashing <= int(max_clashing))

    def residues(self, i: int, pocket) -> list[str]:
        """The residues row i touches, by `pocket`'s labels."""
        return pocket.residues(self.contact_fingerprint[i])

    def atom_label(self, i: int, pocket) -> str:
        """The pocket atom of row i's worst pair (`A:CYS12:SG`); '' without a pair."""
        return pocket.atom_label(int(self.worst[i, 1]))

    def similarity(self, other: "ClashReport | None" = None) -> np.ndarray:
        """Tanimoto similarity of the contact fingerprints, on the GPU (`fingerprint_similarity`)."""
        return fingerprint_similarity(self.contact_fingerprint, None if other is None else other.contact_fingerprint, device=self.device)

    def leaders(self, threshold: float = 0.7, max_leaders: int = 2048):
        """Sphere exclusion over the rows in their order by contact fingerprint (`fingerprint_leaders`): (leaders, leader_of)."""
        return fingerprint_leaders(self.contact_fingerprint, threshold=threshold, max_leaders=max_leaders, device=self.device)


class _PocketHandle(_DeviceHandle):
    _destroy = "pmx_pocket_destroy"

    def __init__(self, pocket, device: int):
        handle = ctypes.c_void_p()
        xyz, radius, group = (np.ascontiguousarray(pocket.xyz, dtype=np.float32), np.ascontiguousarray(pocket.radius, dtype=np.float32),
                              np.ascontiguousarray(pocket.group, dtype=np.uint16))
        n = len(radius)
        _ffi.check(_ffi.load().pmx_pocket_create(xyz.ctypes.data if n else None, radius.ctypes.data if n else None, group.ctypes.data if n else None, n, device,
                                                 ctypes.byref(handle)))
        super().__init__(handle, device)


def device_pocket(pocket, device=None) -> _PocketHandle:
    """The device copy of a `pocket.PocketAtoms`, made once per (pocket, device) and freed with the object."""
    return _cached_handle(pocket._device, _device_index(device), lambda dev: _PocketHandle(pocket, dev))


class _PoseRows:
    """The rows the pose calls share: motions and one source of points, checked and laid out as `pmx_pose_clash`, `pmx_pose_refine`,
    `pmx_pose_shape` and `pmx_shape_overlay` take them. `what` names the caller in a message. `both` (`pmx_combo_overlay`): the rows are
    library ligands - node mode - and may carry a shape source next to their nodes, an atom store or `points` / `point_radii`."""

    def __init__(self, what, library, indices, conformers, rotation, translation, points, point_radii, atoms=None, both=False):
        self.rot = np.ascontiguousarray(np.asarray(rotation, dtype=np.float64).reshape(-1, 3, 3))
        self.trans = np.ascontiguousarray(np.asarray(translation, dtype=np.float64).reshape(-1, 3))
        n = self.n = len(self.rot)
        if len(self.trans) != n:
            raise ValueError("rotation and translation differ in length")
        if n > 65536:
            raise ValueError(f"at most 65536 rows per {what} call (PMX_EXPLAIN_MAX)")
        self.node_mode = library is not None
        self.store = atoms  # a `DeviceAtoms` / `PackedAtoms`: point mode, the points gathered on the device
        if atoms is not None and not _is_store(atoms):
            raise TypeError(f"{what}: atoms is a DeviceAtoms or a PackedAtoms")
        if both:
            if not self.node_mode or (atoms is not None and points is not None):
                raise ValueError(f"{what}: a library, and next to it an atom store or points - at most one of the two")
        elif atoms is not None:
            if self.node_mode or points is not None or point_radii is not None:
                raise ValueError(f"{what}: a library, points or an atom store - exactly one source of points")
        elif self.node_mode == (points is not None):
            raise ValueError(f"{what}: a library with indices and conformers, or points - one of the two")
        self.idx = self.conf = self.off = self.flat = self.rad = self.gstatus = None
        if self.node_mode or atoms is not None:
            self.idx = np.ascontiguousarray(np.asarray(indices, dtype=np.int64).reshape(-1))
            self.conf = np.ascontiguousarray(np.clip(np.asarray(conformers, dtype=np.int64).reshape(-1), -1, 2**31 - 1).astype(np.int32))
            if len(self.idx) != n or len(self.conf) != n:
                raise ValueError("indices, conformers and the motions differ in length")
            if (self.idx < 0).any():
                raise ValueError("negative ligand index")
        if points is not None:
            if len(points) != n:
                raise ValueError(f"{len(points)} point sets for {n} motions")
            self.off, self.flat, pts = _ragged(points, np.float32, 3)
            if point_radii is not None:
                if len(point_radii) != n:
                    raise ValueError(f"{len(point_radii)} radius lists for {n} point sets")
                _, self.rad, rs = _ragged(point_radii, np.float32, None)
                if any(len(r) != len(p) for r, p in zip(rs, pts)):
                    raise ValueError("a list of radii differs in length from its points")

    def upload(self, tdev, dat: "DeviceAtoms | None" = None):
        """The device tensors (kept alive by the caller) and the seven source and motion arguments that follow the pocket and the library:
        ligands and conformers in node mode, offsets, points and radii where the rows have points - in `both` mode all five.
        With an atom store (`dat`, resident on `tdev`) the points are gathered there; a row whose gather status is not OK has no points and
        gets a motion of NaN, so that the call reports it as it reports any row that is not OK (`finish` puts the gather's status in)."""
        torch = _torch()
        n = self.n
        up = lambda a: torch.from_numpy(a).to(tdev)  # noqa: E731
        t_rot, t_trans = up(self.rot.reshape(-1, 9) if n else np.zeros((1, 9))), up(self.trans if n else np.zeros((1, 3)))
        ligands = points = ()
        if self.idx is not None:
            ligands = (up(self.idx if n else np.zeros(1, np.int64)), up(self.conf if n else np.zeros(1, np.int32)))
        if dat is not None:
            *points, self.gstatus = dat.gather_device(*ligands, n)
            t_rot, t_trans = self.not_ok(t_rot, t_trans)
            self.slots, self._off_dev = max(n * dat.max_atoms, 1), points[0]
        elif self.off is not None:
            points = (up(self.off), up(self.flat), up(self.rad) if self.rad is not None else None)
        ptr = lambda ts, k: tuple(None if t is None else t.data_ptr() for t in ts) or (None,) * k  # noqa: E731
        return (t_rot, t_trans, *ligands, *points), ptr(ligands if self.node_mode else (), 2) + ptr(points, 3), (t_rot.data_ptr(), t_trans.data_ptr())

    def not_ok(self, *tensors):
        """Store mode, after the gather: the [n, k] float tensors with NaN in the rows the store has no points for. This is the one place
        such a row is made not OK - NaN in its motion makes every call report it as it reports any row that is not OK."""
        if self.gstatus is None or not self.n:
            return tensors
        bad = (self.gstatus != 0)[:, None]
        return tuple(t.masked_fill(bad, float("nan")) for t in tensors)

    def finish(self, status: np.ndarray) -> np.ndarray:
        """After the wait: the rows' statuses with the gather's where that is not OK, and - store mode - the offsets of the rows' points."""
        if self.gstatus is None:
            return status
        self.off = self._off_dev.cpu().numpy().astype(np.int64)
        g = self.gstatus.cpu().numpy()[: self.n].astype(np.int32)
        return np.where(g != 0, g, status).astype(np.int32)


def _ragged(lists, dtype, width):
    """(offsets int64 [n + 1], the rows back to back and never empty, the rows) of a list of arrays of [m_i, width] (or [m_i] for width None)."""
    rows = [np.asarray(p, dtype=dtype).reshape((-1, width) if width else (-1,)) for p in lists]
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(p) for p in rows])
    flat = np.ascontiguousarray(np.concatenate(rows + [np.zeros((1, width) if width else 1, dtype)]))  # (never an empty buffer)
    return off, flat, rows


class _PoseFrame:
    """What the body of a pose call works with inside `_pose_frame`: `lib` (libpmx), `owner` (the device handle the rows are judged against),
    `library` (the resident library's handle, None outside node mode), `src` and `motion` (the source and motion arguments of the C ABI),
    `n` rows, `m` = max(n, 1) rows to allocate, `slots` per-point outputs to allocate, `status` (int32 [m]), `stream` (a c_void_p), `dev` /
    `tdev`, and `keep` - uploads of the body's own go there to live until the wait. After the block: `st`, the rows' statuses on the host
    and - `per_point` - `lo`, `hi`, where each row's per-point outputs begin and end."""

    def __init__(self, torch, tdev):
        self._torch, self.tdev, self.keep = torch, tdev, []

    def f64(self, *shape):
        return self._torch.empty(shape, dtype=self._torch.float64, device=self.tdev)

    def i32(self, *shape):
        return self._torch.empty(shape, dtype=self._torch.int32, device=self.tdev)

    def i64(self, *shape):
        return self._torch.empty(shape, dtype=self._torch.int64, device=self.tdev)

    def up(self, array):
        """A host array on the device, alive until the wait."""
        self.keep.append(self._torch.from_numpy(array).to(self.tdev))
        return self.keep[-1]

    def host(self, tensor) -> np.ndarray:
        """The first n rows of an output, on the host."""
        return tensor.cpu().numpy()[: self.n]


@contextlib.contextmanager
def _pose_frame(rows: _PoseRows, library, atoms, device, owner, owned, per_point: bool = False):
    """The part the pose calls share, around the one C call that is their own: the library and the atom store made resident (the two
    together for rows of `both` sources: `f.library` and all of `f.src` are set), the device they name, the handle `owner(owned, device)` (`device_pocket`, `device_shape_ref`, `device_model`), the rows uploaded; then the
    body, which allocates its outputs and enqueues its call on torch's current stream; then the wait, the release of the uploads and the
    rows' statuses. A new pose call is an argument check, its outputs, one `_ffi` call, its result."""
    torch = _torch()
    n = rows.n
    with contextlib.ExitStack() as stack:
        dlib = stack.enter_context(_resident(library, device)) if rows.node_mode else None
        dev = dlib.device if rows.node_mode else atoms.device if isinstance(atoms, DeviceAtoms) else _device_index(device)
        dat = stack.enter_context(_resident_atoms(atoms, dev)) if atoms is not None else None
        f = _PoseFrame(torch, torch.device("cuda", dev))
        f.lib, f.owner, f.library, f.rows, f.dev, f.n, f.m = _ffi.load(), owner(owned, dev), dlib.handle if rows.node_mode else None, rows, dev, n, max(n, 1)
        with torch.cuda.device(f.tdev):
            keep, f.src, f.motion = rows.upload(f.tdev, dat)
            f.slots = f.m * _MAX_NODES if rows.node_mode else rows.slots if dat is not None else max(int(rows.off[-1]), 1)
            f.status = f.i32(f.m)
            stream = torch.cuda.current_stream(f.tdev)
            f.stream = ctypes.c_void_p(stream.cuda_stream)
            yield f
            stream.synchronize()
            del keep
            f.keep.clear()
        f.st = rows.finish(f.host(f.status).astype(np.int32))
        if per_point and rows.node_mode:
            f.lo = np.arange(n, dtype=np.int64) * _MAX_NODES
            f.hi = f.lo + np.where(f.st != 1, _record_counts(dlib, rows.idx, 0), 0)
        elif per_point:
            f.lo, f.hi = rows.off[:-1], rows.off[1:]


def clashes(pocket, library=None, indices=None, conformers=None, rotation=None, translation=None, points=None, point_radii=None, node_radius: float = 1.0,
            tolerance: float = 0.5, contact: float = 4.5, device=None, atoms=None) -> ClashReport:
    """Posed rows against the pocket's atoms (`pmx_pose_clash`, csrc/pmx_pocket.hip): row i is a set of points moved by `rotation[i]`
    [3, 3] and `translation[i]` [3] - what `Alignment` holds - and a pair (point, atom) clashes when the two spheres overlap by more than
    `tolerance`, touches when the centres are closer than `contact`.
      node mode   `library` (a `DeviceLibrary` or anything `as_packed_library` accepts), `indices`, `conformers`: the pharmacophore nodes of
                  library ligand indices[i] at conformer conformers[i], each a sphere of `node_radius`
      point mode  `points`: a list of [m_i, 3] arrays, any points of the conformer's frame - a whole molecule's atoms; `point_radii`: a
                  matching list of radii (`pocket.atomic_number_radii` makes them from atomic numbers), or None for `node_radius` each
      atom store  `atoms` (a `DeviceAtoms`, or a `PackedAtoms` uploaded for the call), `indices`, `conformers`: the heavy atoms of ligand
                  indices[i] at conformer conformers[i] with Bondi radii, gathered on the device (`pmx_atoms_gather`) - point mode without
                  host arrays. A row the store has no atoms for (status 1), or whose conformer the record lacks (status 4), is not OK
    Exactly one of the three. At most 65536 rows. Runs on torch's current stream of the device and waits for it."""
    _torch()
    rows = _PoseRows("clashes", library, indices, conformers, rotation, translation, points, point_radii, atoms)
    with _pose_frame(rows, library, atoms, device, device_pocket, pocket, per_point=True) as f:
        summary, count, ppen, patom, fp = f.f64(f.m, 4), f.i32(f.m, 6), f.f64(f.slots), f.i32(f.slots), f.i64(f.m, _FP_WORDS)
        _ffi.check(f.lib.pmx_pose_clash(f.owner.handle, f.library, *f.src, *f.motion, f.n, float(node_radius), float(tolerance), float(contact), summary.data_ptr(),
                                        count.data_ptr(), ppen.data_ptr(), patom.data_ptr(), fp.data_ptr(), f.status.data_ptr(), f.stream))
    n, lo, hi, st, dev = f.n, f.lo, f.hi, f.st, f.dev
    sm, cn = f.host(summary), f.host(count).astype(np.int64)
    pp, pa = ppen.cpu().numpy(), patom.cpu().numpy().astype(np.int64)
    return ClashReport(clearance=sm[:, 0].copy(), overlap=sm[:, 1].copy(), n_points=cn[:, 0].copy(), n_clashing=cn[:, 1].copy(), n_pairs=cn[:, 2].copy(),
                       n_contacts=cn[:, 3].copy(), worst=cn[:, 4:6].copy(), point_penetration=[pp[lo[i]: hi[i]].copy() for i in range(n)],
                       point_atom=[pa[lo[i]: hi[i]].copy() for i in range(n)], contact_fingerprint=f.host(fp).view(np.uint64).copy(), status=st, device=dev)


@dataclass
class ShapeReport:
    """What `shape` returns: one row per posed set of points against a reference ligand (definitions: `pmx_pose_shape` in include/pmx.h).
    Floats are float64.

    overlap[i], self_overlap[i], reference_overlap[i]   O_AB, O_AA, O_BB: the first-order Gaussian overlap volumes (row with reference, row
                    with itself, reference with itself), A^3. They over-count a molecule's volume; the ratios below largely cancel that
    tanimoto[i]     O_AB / (O_AA + O_BB - O_AB): the shape Tanimoto, exactly 1 for the reference's own atoms in place
    reference_fraction[i]   O_AB / O_BB: how much of the known ligand the row fills
    fit_fraction[i]         O_AB / O_AA: how much of the row lies inside the known ligand
    rms_to_reference[i]     the root mean square, over the row's points, of the distance to the nearest reference atom (NaN without a point)
    rms_from_reference[i]   the same over the reference atoms, to the nearest point of the row (+inf without a point)
    rmsd_in_order[i]        atom-for-atom RMSD, point a against reference atom a, where the row has exactly as many points as the
                    reference has atoms - the same molecule in the same atom order - and NaN otherwise
    n_points[i], n_covered[i], n_reference_covered[i]   points, points within `cover` of a reference atom, reference atoms within `cover`
                    of a point
    point_distance[i], point_reference_atom[i]   per point the distance to its nearest reference atom, and that atom
    reference_distance[i], reference_point[i]    per reference atom the distance to the row's nearest point, and that point
    status[i]       0, 1 (PMX_LIGAND_UNSUPPORTED) or 4 (PMX_LIGAND_KEY_INVALID: not a conformer of the ligand, a motion that is not
                    finite, a radius that is not a finite number > 0); such a row has NaN, zero counts and -1"""

    overlap: np.ndarray
    self_overlap: np.ndarray
    reference_overlap: np.ndarray
    tanimoto: np.ndarray
    reference_fraction: np.ndarray
    fit_fraction: np.ndarray
    rms_to_reference: np.ndarray
    rms_from_reference: np.ndarray
    rmsd_in_order: np.ndarray
    n_points: np.ndarray
    n_covered: np.ndarray
    n_reference_covered: np.ndarray
    point_distance: list
    point_reference_atom: list
    reference_distance: list
    reference_point: list
    status: np.ndarray

    def __len__(self) -> int:
        return len(self.status)


class _ShapeRefHandle(_DeviceHandle):
    _destroy = "pmx_shape_ref_destroy"

    def __init__(self, reference, device: int):
        handle = ctypes.c_void_p()
        xyz, radius = np.ascontiguousarray(reference.xyz, dtype=np.float32), np.ascontiguousarray(reference.radius, dtype=np.float32)
        _ffi.check(_ffi.load().pmx_shape_ref_create(xyz.ctypes.data, radius.ctypes.data, len(radius), device, ctypes.byref(handle)))
        super().__init__(handle, device)
        self.m = len(radius)

    @property
    def self_overlap(self) -> float:
        out = ctypes.c_double()
        _ffi.check(_ffi.load().pmx_shape_ref_self(self.handle, ctypes.byref(out)))
        return out.value


def device_shape_ref(reference, device=None) -> _ShapeRefHandle:
    """The device copy of a `shape.ReferenceLigand`, made once per (reference, device) and freed with the object."""
    return _cached_handle(reference._device, _device_index(device), lambda dev: _ShapeRefHandle(reference, dev))


def shape(reference, library=None, indices=None, conformers=None, rotation=None, translation=None, points=None, point_radii=None, atoms=None,
          node_radius: float = 1.0, cover: float = 2.0, device=None) -> ShapeReport:
    """Posed rows against a known ligand (`pmx_pose_shape`, csrc/pmx_pose_shape.hip): row i is a set of points moved by `rotation[i]` and
    `translation[i]` - what `Alignment` holds - and `reference` a `shape.ReferenceLigand` in the pocket's frame. The Gaussian shape overlap
    of the two, its Tanimoto and Tversky ratios, and nearest-atom distances both ways; a point (a reference atom) is covered when its
    nearest counterpart is closer than `cover`. The pose is judged where it is: nothing is moved. The three sources of points - node mode
    (`library`, `indices`, `conformers`, each node a sphere of `node_radius`), point mode (`points`, `point_radii`) and the atom store
    (`atoms`, `indices`, `conformers`) - are those of `clashes`; a row holds at most 256 points. Exactly one of the three. At most 65536
    rows. Runs on torch's current stream of the device and waits for it."""
    _torch()
    rows = _PoseRows("shape", library, indices, conformers, rotation, translation, points, point_radii, atoms)
    with _pose_frame(rows, library, atoms, device, device_shape_ref, reference, per_point=True) as f:
        summary, count, pnear, pref = f.f64(f.m, 10), f.i32(f.m, 4), f.f64(f.slots), f.i32(f.slots)
        rnear, rpoint = f.f64(f.m, _ffi.MAX_LIGAND_ATOMS), f.i32(f.m, _ffi.MAX_LIGAND_ATOMS)
        _ffi.check(f.lib.pmx_pose_shape(f.owner.handle, f.library, *f.src, *f.motion, f.n, float(node_radius), float(cover), summary.data_ptr(), count.data_ptr(),
                                        pnear.data_ptr(), pref.data_ptr(), rnear.data_ptr(), rpoint.data_ptr(), f.status.data_ptr(), f.stream))
    n, lo, hi, st, rm = f.n, f.lo, f.hi, f.st, f.owner.m
    sm, cn = f.host(summary), f.host(count).astype(np.int64)
    pn, pr = pnear.cpu().numpy(), pref.cpu().numpy().astype(np.int64)
    rn, rp = f.host(rnear)[:, :rm], f.host(rpoint)[:, :rm].astype(np.int64)
    return ShapeReport(overlap=sm[:, 0].copy(), self_overlap=sm[:, 1].copy(), reference_overlap=sm[:, 2].copy(), tanimoto=sm[:, 3].copy(),
                       reference_fraction=sm[:, 4].copy(), fit_fraction=sm[:, 5].copy(), rms_to_reference=sm[:, 6].copy(), rms_from_reference=sm[:, 7].copy(),
                       rmsd_in_order=sm[:, 8].copy(), n_points=cn[:, 0].copy(), n_covered=cn[:, 1].copy(), n_reference_covered=cn[:, 2].copy(),
                       point_distance=[pn[lo[i]: hi[i]].copy() for i in range(n)], point_reference_atom=[pr[lo[i]: hi[i]].copy() for i in range(n)],
                       reference_distance=[rn[i].copy() for i in range(n)], reference_point=[rp[i].copy() for i in range(n)], status=st)


@dataclass
class RefinedPoses(_PosedRows, _Overlayable):
    """What `refine` returns: one row per posed set of points (definitions: `pmx_pose_refine` in include/pmx.h). Floats are float64.

    rotation[i], translation[i]   the refined motion: a point x of the conformer sits at R x + t. The input's own bits where nothing clashed
    overlap_start[i], overlap[i]  the overlap (`ClashReport.overlap`) at the input motion and at the refined one
    restraint_start[i], restraint_energy[i]   sum over the anchors of w |R a + t - b|^2, before and after (unscaled by `restraint`)
    anchor_rmsd[i]  sqrt(restraint_energy / sum w): how far the anchors moved off their targets
    angle[i], shift[i]   the net rotation from the input motion in rad, and how far the centroid of the posed points moved
    iterations[i], accepted[i]    evaluations after the first, and the steps among them that lowered the energy
    stop[i]         0 nothing clashed, 1 converged (decrease <= ftol E), 2 out of iterations, 3 no step found (lambda > 1e8); -1 not OK
    n_pairs[i]      clashing pairs at the refined motion
    status[i]       0, 1 (PMX_LIGAND_UNSUPPORTED) or 4 (PMX_LIGAND_KEY_INVALID: not a conformer, a motion that is not finite, a weight
                    that is negative or not finite); such a row has NaN floats, zero counts and stop -1
    indices, conformers   node mode: the rows' ligands and conformers (None in point mode)
    `transform`, `clashes`, `pose_fit`, `shape` and `overlay` of the refined poses, as `Alignment` has them of the fitted ones: see
    `_PosedRows`. A row the refinement left untouched has the bits it had before."""

    rotation: np.ndarray
    translation: np.ndarray
    overlap_start: np.ndarray
    overlap: np.ndarray
    restraint_start: np.ndarray
    restraint_energy: np.ndarray
    anchor_rmsd: np.ndarray
    angle: np.ndarray
    shift: np.ndarray
    iterations: np.ndarray
    accepted: np.ndarray
    stop: np.ndarray
    n_pairs: np.ndarray
    status: np.ndarray
    indices: "np.ndarray | None" = None
    conformers: "np.ndarray | None" = None

    def __len__(self) -> int:
        return len(self.status)


@dataclass
class ShapeOverlay(_PosedRows, _Refinable):
    """What `overlay` returns: one row per hit - the rigid motion that maximises its Gaussian shape overlap with a reference ligand from
    where it started (definitions: `pmx_shape_overlay` and `pmx_shape_starts` in include/pmx.h). Floats are float64. Rigid only, shape
    only (no atom types, no hydrogens), and a local maximum: the one the start leads to.

    rotation[i], translation[i]   the overlaid motion: a point x of the conformer sits at R x + t. The start's own bits where no step was taken
    overlap_start[i], overlap[i]  O_AB at the start motion and at the overlaid one (never lower)
    self_overlap[i], reference_overlap[i]   O_AA and O_BB, which no rigid motion changes
    tanimoto_start[i], tanimoto[i]   O_AB / (O_AA + O_BB - O_AB) before and after
    angle[i], shift[i]   the net rotation from the start in rad, and how far the centroid of the posed points moved
    iterations[i], accepted[i]    trial motions, and the ones among them that raised O_AB
    stop[i]         0 nothing to follow (no point, or O_AB = 0: too far away), 1 converged (increase <= ftol O_AB), 2 out of iterations,
                    3 no step found (lambda > 1e8: a row that starts at a maximum ends so); -1 not OK
    n_points[i]     the row's points
    start[i]        with `starts=4`: which inertial start (0: the frames laid on each other, 1 .. 3: and a half turn about the row's
                    first, second or third axis) was kept - the one of highest final Tanimoto, the lower among equals; -1 with `starts=0`
    start_tanimoto  [n, starts]: every start's final Tanimoto
    status[i]       0, 1 (PMX_LIGAND_UNSUPPORTED) or 4 (PMX_LIGAND_KEY_INVALID); such a row has NaN floats, zero counts and stop -1
    indices, conformers   the rows' ligands and conformers (None for points of the caller's)
    `transform`, `shape`, `clashes`, `refine` and `pose_fit` of the overlaid poses, as `Alignment` has them of the fitted ones: see
    `_PosedRows` (a shape overlay knows nothing of the protein: check it)."""

    rotation: np.ndarray
    translation: np.ndarray
    overlap_start: np.ndarray
    overlap: np.ndarray
    self_overlap: np.ndarray
    reference_overlap: np.ndarray
    tanimoto_start: np.ndarray
    tanimoto: np.ndarray
    angle: np.ndarray
    shift: np.ndarray
    iterations: np.ndarray
    accepted: np.ndarray
    stop: np.ndarray
    n_points: np.ndarray
    start: np.ndarray
    start_tanimoto: np.ndarray
    status: np.ndarray
    indices: "np.ndarray | None" = None
    conformers: "np.ndarray | None" = None

    def __len__(self) -> int:
        return len(self.status)


def overlay(reference, library=None, indices=None, conformers=None, rotation=None, translation=None, points=None, point_radii=None, atoms=None, starts: int = 0,
            node_radius: float = 1.0, ftol: float = 1e-6, max_iter: int = 32, device=None) -> ShapeOverlay:
    """Rows overlaid on a known ligand (`pmx_shape_overlay`, csrc/pmx_shape_overlay.hip): per row a bounded Levenberg-Marquardt
    maximisation over the rigid motion of the Gaussian shape overlap `shape` reports. Rows, points and radii as `shape` takes them (node
    mode, point mode, or an atom store `atoms`).
      starts=0   each row is optimised from its given motion: how far is this pose from its best shape match nearby?
      starts=4   `rotation` / `translation` are ignored and may be None: each hit is run from the four motions that lay its inertial frame
                 on the reference's (`pmx_shape_starts`), and the start of highest final Tanimoto is kept (the lower among equals). At
                 most 16384 hits
      max_iter, ftol  at most `max_iter` (<= 64) trial motions per row; a step that raises O_AB by no more than ftol * O_AB ends the row
    Rigid only, shape only (no atom types, no hydrogens), unweighted inertial frames, and a local maximum. At most 65536 rows. Runs on
    torch's current stream of the device and waits for it."""
    _torch()
    _overlay_check("overlay", starts, max_iter, ftol, node_radius)
    hits = 0 if not starts else len(points) if points is not None else len(np.asarray(indices).reshape(-1))
    indices, conformers, rotation, translation, points, point_radii = _expand_starts("overlay", starts, hits, indices, conformers, rotation, translation, points, point_radii)
    rows = _PoseRows("overlay", library, indices, conformers, rotation, translation, points, point_radii, atoms)
    with _pose_frame(rows, library, atoms, device, device_shape_ref, reference) as f:
        rot, trans, energy, count = f.f64(f.m, 3, 3), f.f64(f.m, 3), f.f64(f.m, 8), f.i32(f.m, 4)
        _ffi.check(f.lib.pmx_shape_overlay(f.owner.handle, f.library, *f.src, *_start_motion(f, starts), f.n, float(node_radius), float(ftol), int(max_iter), rot.data_ptr(),
                                           trans.data_ptr(), energy.data_ptr(), count.data_ptr(), f.status.data_ptr(), f.stream))
    st = f.st
    en, cn, R, t = f.host(energy), f.host(count).astype(np.int64), f.host(rot), f.host(trans)
    pick, start, start_tanimoto = _pick_start(en[:, 5], starts)
    has_rows = rows.node_mode or atoms is not None
    return ShapeOverlay(rotation=R[pick].copy(), translation=t[pick].copy(), overlap_start=en[pick, 0], overlap=en[pick, 1], self_overlap=en[pick, 2],
                        reference_overlap=en[pick, 3], tanimoto_start=en[pick, 4], tanimoto=en[pick, 5], angle=en[pick, 6], shift=en[pick, 7], iterations=cn[pick, 0],
                        accepted=cn[pick, 1], stop=cn[pick, 2], n_points=cn[pick, 3], start=start, start_tanimoto=start_tanimoto, status=st[pick],
                        indices=rows.idx[pick].copy() if has_rows else None, conformers=rows.conf[pick].astype(np.int64) if has_rows else None)


@dataclass
class ShapeStarts:
    """What `overlay_starts` returns (definitions: `pmx_shape_starts` in include/pmx.h): per row the start motion `rotation[i]`,
    `translation[i]`, and the row's own inertial frame - `centre[i]` [3], `axes[i]` [3, 3] (axis k is row k; right-handed, by descending
    `values[i]` [3], the sums of squares along them) - for a caller who wants another set of starts. A row that is not OK (`status[i]`
    1 or 4; 4 also for a start outside 0 .. 3) has NaN."""

    rotation: np.ndarray
    translation: np.ndarray
    centre: np.ndarray
    axes: np.ndarray
    values: np.ndarray
    status: np.ndarray

    def __len__(self) -> int:
        return len(self.status)


def _shape_starts(f: _PoseFrame, which, status):
    """`pmx_shape_starts` of a frame's rows, enqueued: start `which[i]` (an int32 device tensor) of row i. Returns the device tensors
    (rotation [m, 9], translation [m, 3], frame [m, 16]), NaN in a row the store has no atoms for, whatever its empty point list gave;
    `status` takes the call's statuses. Behind `overlay_starts` and the inertial leg of `overlay(starts=4)` and `combo_overlay(starts=4)`;
    rows that carry shape points next to their nodes start by those points, so the call gets them alone."""
    rot, trans, frame = f.f64(f.m, 9), f.f64(f.m, 3), f.f64(f.m, 16)
    library, src = (None, (None, None, *f.src[2:4])) if f.src[2] is not None else (f.library, f.src[:4])
    _ffi.check(f.lib.pmx_shape_starts(f.owner.handle, library, *src, which.data_ptr(), f.n, rot.data_ptr(), trans.data_ptr(), frame.data_ptr(), status.data_ptr(), f.stream))
    out = f.rows.not_ok(rot, trans, frame)
    f.keep += [which, status, *out]
    return out


def _start_motion(f: _PoseFrame, starts: int):
    """The motion arguments an overlay starts from: the frame's own, or - row i being start i % starts of its hit - the inertial ones."""
    if not starts:
        return f.motion
    rot, trans, _ = _shape_starts(f, _torch().arange(f.m, dtype=_torch().int32, device=f.tdev) % starts, f.i32(f.m))
    return rot.data_ptr(), trans.data_ptr()


def _overlay_check(what, starts, max_iter, ftol, node_radius) -> None:
    """The arguments `overlay` and `combo_overlay` have in common."""
    if starts not in (0, 4):
        raise ValueError(f"{what}: starts is 0 (from the given motions) or 4 (the inertial starts)")
    if not 0 <= int(max_iter) <= 64:
        raise ValueError("max_iter: 0 to 64 (PMX_REFINE_MAX_ITER)")
    if not (np.isfinite(ftol) and ftol >= 0):
        raise ValueError("ftol must be finite and not negative")
    if not np.isfinite(node_radius):
        raise ValueError("node_radius must be finite")


def _expand_starts(what, starts, hits, indices, conformers, rotation, translation, points, point_radii):
    """The rows of an overlay from `starts` starts a hit: (indices, conformers, rotation, translation, points, point_radii) with every hit
    `starts` times in a row under a motion of zeros (the inertial starts replace it); as they are with `starts=0`, which needs motions."""
    if not starts:
        if rotation is None or translation is None:
            raise ValueError(f"{what}: starts=0 optimises the given motions - rotation and translation")
        return indices, conformers, rotation, translation, points, point_radii
    if hits > 16384:
        raise ValueError(f"{what}: {hits} hits, at most 16384 with starts={starts} (65536 rows)")
    rep = lambda v: None if v is None else [x for x in v for _ in range(starts)]  # noqa: E731
    if indices is not None:
        indices, conformers = np.repeat(np.asarray(indices).reshape(-1), starts), np.repeat(np.asarray(conformers).reshape(-1), starts)
    return indices, conformers, np.zeros((hits * starts, 3, 3)), np.zeros((hits * starts, 3)), rep(points), rep(point_radii)


def _pick_start(column: np.ndarray, starts: int):
    """(pick, start, values) of the rows' final values `column`: per hit the row of its best start - the highest value, the first among
    equals, NaN below everything -, which start that is, and every start's value [hits, starts]. With `starts=0` every row is its own hit."""
    n = len(column)
    if not starts:
        return np.arange(n), np.full(n, -1, np.int64), np.zeros((n, 0))
    each = column.reshape(n // starts, starts)
    best = np.argmax(np.where(np.isnan(each), -np.inf, each), axis=1) if len(each) else np.zeros(0, np.int64)
    return np.arange(len(each)) * starts + best, best.astype(np.int64), each.copy()


def overlay_starts(reference, start, library=None, indices=None, conformers=None, points=None, atoms=None, device=None) -> ShapeStarts:
    """The inertial start motions of rows (`pmx_shape_starts`): row i's points - as `overlay` takes them - laid with their unweighted
    inertial frame on the reference's, start[i] = 0, or 1 .. 3 for a further half turn about the row's first, second or third axis. What
    `overlay(..., starts=4)` runs from. At most 65536 rows."""
    _torch()
    start = np.ascontiguousarray(np.clip(np.asarray(start, dtype=np.int64).reshape(-1), -1, 2**31 - 1).astype(np.int32))
    n = len(start)
    rows = _PoseRows("overlay_starts", library, indices, conformers, np.zeros((n, 3, 3)), np.zeros((n, 3)), points, None, atoms)
    with _pose_frame(rows, library, atoms, device, device_shape_ref, reference) as f:
        rot, trans, frame = _shape_starts(f, f.up(start if n else np.zeros(1, np.int32)), f.status)
    R, t, fr, st = f.host(rot).reshape(-1, 3, 3).copy(), f.host(trans).copy(), f.host(frame).copy(), f.st
    return ShapeStarts(rotation=R, translation=t, centre=fr[:, 0:3].copy(), axes=fr[:, 3:12].reshape(-1, 3, 3).copy(), values=fr[:, 12:15].copy(), status=st)


def _heavy_atoms(atoms, conformers):
    """Per row the heavy atoms of `atoms[i]` (a `LigandFeatures` / `Ligand`) at conformer `conformers[i]`, float32 [m_i, 3], and their
    Bondi radii by atomic number. Hydrogens are left out (the pocket's are not read either); a row whose conformer the molecule does not have
    gets no point (its status says so already)."""
    from .pocket import atomic_number_radii

    points, radii = [], []
    for mol, c in zip(atoms, conformers):
        pos = np.asarray(mol.atom_positions, dtype=np.float32)  # [n_atoms, C, 3]
        c = int(c)
        z = _atomic_numbers(mol)
        heavy = z > 1
        points.append(pos[heavy, c] if 0 <= c < pos.shape[1] else np.zeros((0, 3), np.float32))
        radii.append(atomic_number_radii(z[heavy])[: len(points[-1])])
    return points, radii


def _pose_source(poses, what, pocket_or_model, library, atoms):
    """(pocket, the keyword arguments that name the points of `poses`' rows for `clashes` / `refine`): node mode with `library` alone,
    point mode - the molecules' heavy atoms - with `atoms`: a list of molecules, one per row, or the library's atom store
    (`DeviceAtoms` / `PackedAtoms`)."""
    from .pocket import PocketAtoms

    # (`shape` judges the rows against a reference ligand: no pocket)
    pocket = pocket_or_model if pocket_or_model is None or isinstance(pocket_or_model, PocketAtoms) else pocket_or_model.pocket_atoms()
    if atoms is None:
        if library is None:
            raise ValueError(f"{what}: the library the rows are ligands of, or `atoms`")
        return pocket, dict(library=library, indices=poses.indices, conformers=poses.conformers)
    if poses.conformers is None:
        raise ValueError(f"{what}: these rows have no conformers to take the atoms at")
    if _is_store(atoms):  # the rows' atoms are gathered on the device, from the store that goes with the rows' library
        return pocket, dict(atoms=atoms, indices=poses.indices, conformers=poses.conformers)
    if len(atoms) != len(poses):
        raise ValueError(f"{len(atoms)} molecules for {len(poses)} rows")
    points, radii = _heavy_atoms(atoms, poses.conformers)
    return pocket, dict(points=points, point_radii=radii)


def refine(pocket, library=None, indices=None, conformers=None, rotation=None, translation=None, points=None, point_radii=None, anchors=None, anchor_targets=None,
           anchor_weights=None, node_radius: float = 1.0, tolerance: float = 0.5, restraint: float = 0.1, max_iter: int = 32, ftol: float = 1e-9,
           device=None, atoms=None) -> RefinedPoses:
    """Posed rows moved out of the pocket's atoms (`pmx_pose_refine`, csrc/pmx_refine.hip): per row a bounded Levenberg-Marquardt
    minimisation over the rigid motion of the overlap `clashes` reports plus `restraint` times a harmonic term that holds the row's anchors
    where the input motion put them. Rows, points and radii as `clashes` takes them (node mode, point mode, or an atom store `atoms`).
      anchors         None: the row's own points, each of weight 1. Otherwise a list of [k_i, 3] arrays in the conformer's frame
      anchor_targets  a matching list of [k_i, 3] float64 positions in the pocket's frame (default: the anchors under the input motion)
      anchor_weights  a matching list of [k_i] weights >= 0 (default 1 each)
      restraint       the weight of the restraint against the overlap, both in A^2. The default 0.1 is uncalibrated: nobody has measured
                      which value separates a grazed side chain from a pierced backbone best; DESIGN.md has what is known
      max_iter, ftol  at most `max_iter` (<= 64) trial motions per row; a step that lowers the energy by no more than ftol * E ends the row
    A penalty on the overlap balanced against a restraint never reaches an overlap of exactly zero: to make a pose pass a check at
    `tolerance`, refine at a smaller one. At most 65536 rows. Runs on torch's current stream of the device and waits for it."""
    _torch()
    rows = _PoseRows("refine", library, indices, conformers, rotation, translation, points, point_radii, atoms)
    n, node_mode = rows.n, rows.node_mode
    if not 0 <= int(max_iter) <= 64:
        raise ValueError("max_iter: 0 to 64 (PMX_REFINE_MAX_ITER)")
    if not (np.isfinite(restraint) and restraint >= 0 and np.isfinite(ftol) and ftol >= 0):
        raise ValueError("restraint and ftol must be finite and not negative")
    a_off = a_flat = a_tgt = a_wts = None
    if anchors is None:
        if anchor_targets is not None or anchor_weights is not None:
            raise ValueError("refine: anchor_targets and anchor_weights go with anchors")
    else:
        if len(anchors) != n:
            raise ValueError(f"{len(anchors)} anchor sets for {n} motions")
        a_off, a_flat, arows = _ragged(anchors, np.float32, 3)
        for name, given, width in (("anchor_targets", anchor_targets, 3), ("anchor_weights", anchor_weights, None)):
            if given is None:
                continue
            if len(given) != n:
                raise ValueError(f"{len(given)} lists of {name} for {n} anchor sets")
            _, flat, rs = _ragged(given, np.float64, width)
            if any(len(r) != len(p) for r, p in zip(rs, arows)):
                raise ValueError(f"a list of {name} differs in length from its anchors")
            if width:
                a_tgt = flat
            else:
                a_wts = flat
    with _pose_frame(rows, library, atoms, device, device_pocket, pocket) as f:
        anchor = [None if a is None else f.up(a).data_ptr() for a in (a_off, a_flat, a_tgt, a_wts)]
        rot, trans, energy, count = f.f64(f.m, 3, 3), f.f64(f.m, 3), f.f64(f.m, 8), f.i32(f.m, 4)
        _ffi.check(f.lib.pmx_pose_refine(f.owner.handle, f.library, *f.src, *anchor, *f.motion, n, float(node_radius), float(tolerance), float(restraint), float(ftol),
                                         int(max_iter), rot.data_ptr(), trans.data_ptr(), energy.data_ptr(), count.data_ptr(), f.status.data_ptr(), f.stream))
    en, cn = f.host(energy), f.host(count).astype(np.int64)
    return RefinedPoses(rotation=f.host(rot).copy(), translation=f.host(trans).copy(), overlap_start=en[:, 0].copy(), overlap=en[:, 2].copy(),
                        restraint_start=en[:, 1].copy(), restraint_energy=en[:, 3].copy(), anchor_rmsd=en[:, 4].copy(), angle=en[:, 5].copy(), shift=en[:, 6].copy(),
                        iterations=cn[:, 0].copy(), accepted=cn[:, 1].copy(), stop=cn[:, 2].copy(), n_pairs=cn[:, 3].copy(),
                        status=f.st, indices=rows.idx.copy() if node_mode else None,
                        conformers=rows.conf.astype(np.int64) if node_mode else None)


@dataclass
class PoseFit:
    """What `pose_fit` returns: one row per posed ligand - the Gaussian overlap of its posed pharmacophore nodes with the model's hotspots,
    each hotspot's radius its positional sigma (definitions: `pmx_pose_fit` in include/pmx.h). Floats are float64. Not a docking score: no
    direction, no atoms, and not the reference's score.

    fit[i], ideal[i]        the sum over the nodes of the mean of w exp(-z^2 / 2) over a node's pairs, and the same with every z = 0
    fraction[i]             fit / ideal: 1.0 with every node on all its hotspots; 0 where ideal is 0
    best_fit[i], best_ideal[i], best_fraction[i]   the same over each node's nearest hotspot (smallest z) alone
    n_nodes[i], n_pairs[i]  nodes with a pair, and pairs    n_in_place[i]  nodes most of whose pairs pass (|z| < 2)    n_passing[i]  passing pairs
    node_fit[i], node_best[i], node_z2[i], node_target[i]   [n] per node of the record: its mean, its nearest hotspot's term, that z^2 and that
                            model node; -1 for a node without a pair
    hotspot_z2[i], hotspot_node[i]   [Nm] per model node: the smallest z^2 of a pair with it (+inf without one) and the ligand node (-1)
    occupied_fingerprint    uint64 [n, 4]: bit m says some pair with model node m passes
    status[i]               0, 1 (PMX_LIGAND_UNSUPPORTED) or 4 (PMX_LIGAND_KEY_INVALID: not a conformer, a motion that is not finite - a
                            row of an `Alignment` that was not OK -, a match that is no candidate); such a row has NaN floats, zero counts,
                            -1 targets and an empty fingerprint"""

    indices: np.ndarray
    conformers: np.ndarray
    fit: np.ndarray
    ideal: np.ndarray
    fraction: np.ndarray
    best_fit: np.ndarray
    best_ideal: np.ndarray
    best_fraction: np.ndarray
    n_nodes: np.ndarray
    n_pairs: np.ndarray
    n_in_place: np.ndarray
    n_passing: np.ndarray
    node_fit: list
    node_best: list
    node_z2: list
    node_target: list
    hotspot_z2: list
    hotspot_node: list
    occupied_fingerprint: np.ndarray
    status: np.ndarray
    device: "int | None" = None  # where `similarity` and `leaders` run

    def __len__(self) -> int:
        return len(self.status)

    def occupied(self, i: int) -> np.ndarray:
        """The model nodes row i occupies (the set bits of its fingerprint), ascending."""
        bits = np.unpackbits(np.ascontiguousarray(self.occupied_fingerprint[i]).view(np.uint8), bitorder="little")
        return np.flatnonzero(bits).astype(np.int64)

    def coverage(self, i: int, model, weights: dict[str, float] | None = None) -> float:
        """The occupied model nodes over the model nodes of positive weight (0.0 where no node has weight)."""
        w = np.asarray(weights_vector(weights), dtype=np.float32)[np.asarray(model.flat.node_type, dtype=np.int64)[: model.num_nodes]]
        total = int(np.count_nonzero(w > 0))
        return len(self.occupied(i)) / total if total else 0.0

    def similarity(self, other: "PoseFit | None" = None) -> np.ndarray:
        """Tanimoto similarity of the occupied-hotspot fingerprints, on the GPU (`fingerprint_similarity`)."""
        return fingerprint_similarity(self.occupied_fingerprint, None if other is None else other.occupied_fingerprint, device=self.device)

    def leaders(self, threshold: float = 0.7, max_leaders: int = 2048):
        """Sphere exclusion over the rows in their order by occupied hotspots (`fingerprint_leaders`): (leaders, leader_of)."""
        return fingerprint_leaders(self.occupied_fingerprint, threshold=threshold, max_leaders=max_leaders, device=self.device)


def _ratio(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """a / b in float64, 0 where b is 0 (NaN stays NaN)."""
    out = np.zeros_like(a)
    np.divide(a, b, out=out, where=b != 0)
    return out


def pose_fit(model, library, indices, conformers, rotation, translation, keys=None, weights: dict[str, float] | None = None, centers=None, sigmas=None,
             device=None) -> PoseFit:
    """Posed library ligands against the model's hotspots (`pmx_pose_fit`, csrc/pmx_pose_fit.hip): row i is the pharmacophore nodes of
    library ligand indices[i] at conformer conformers[i], moved by `rotation[i]` [3, 3] and `translation[i]` [3] - what `Alignment` and
    `RefinedPoses` hold.
      keys      None (free mode): a node pairs with every model node of a type it has. Otherwise the rows' keys as `align` takes them (key
                mode): the pairs are `align`'s for that key
      centers, sigmas   float64 [Nm, 3] / [Nm] in place of the model nodes' `center` and `radius`: "what if this hotspot were tighter". A
                sigma that is not a finite number > 0 takes its model node out
    At most 65536 rows. Runs on torch's current stream of the device and waits for it."""
    _torch()
    rows = _PoseRows("pose_fit", library, indices, conformers, rotation, translation, None, None)
    n = rows.n
    nm = int(model.num_nodes)
    kb = None
    if keys is not None:
        from .engine import _listed_rows  # (the keys as `align` takes them)

        _, _, kb = _listed_rows(rows.idx, rows.conf, keys, "pose_fit")
    over = []
    for name, given, shape in (("centers", centers, (nm, 3)), ("sigmas", sigmas, (nm,))):
        if given is None:
            over.append(None)
            continue
        arr = np.ascontiguousarray(np.asarray(given, dtype=np.float64))
        if arr.shape != shape:
            raise ValueError(f"pose_fit: {name} of shape {arr.shape}, the model has {nm} nodes ({shape})")
        over.append(np.concatenate([arr.reshape(-1), np.zeros(3)]))  # (never an empty buffer)
    with _pose_frame(rows, library, None, device, device_model, model, per_point=True) as f:
        t_cen = f.owner.node_centers(model) if over[0] is None else f.up(over[0])
        t_sig = f.owner.node_sigmas(model) if over[1] is None else f.up(over[1])
        t_key = None if kb is None else f.up(kb).data_ptr()
        m = f.m
        summary, count, fp = f.f64(m, 4), f.i32(m, 4), f.i64(m, _FP_WORDS)
        nfit, nbest, nz2, ntgt = f.f64(m, _MAX_NODES), f.f64(m, _MAX_NODES), f.f64(m, _MAX_NODES), f.i32(m, _MAX_NODES)
        hz2, hnode = f.f64(m, _MAX_MODEL_NODES), f.i32(m, _MAX_MODEL_NODES)
        _ffi.check(f.lib.pmx_pose_fit(f.owner.handle, f.library, _weights_array(weights), t_cen.data_ptr(), t_sig.data_ptr(), f.src[0], f.src[1], t_key, *f.motion, n,
                                      summary.data_ptr(), count.data_ptr(), nfit.data_ptr(), nbest.data_ptr(), nz2.data_ptr(), ntgt.data_ptr(), hz2.data_ptr(), hnode.data_ptr(),
                                      fp.data_ptr(), f.status.data_ptr(), f.stream))
    st, dev, nn = f.st, f.dev, f.hi - f.lo
    sm, cn = f.host(summary), f.host(count).astype(np.int64)
    cut = lambda t, w, dt=None: [(a[: w[i]].copy() if dt is None else a[: w[i]].astype(dt)) for i, a in enumerate(t.cpu().numpy()[:n])]  # noqa: E731
    wm = np.full(n, nm, dtype=np.int64)
    return PoseFit(indices=rows.idx.astype(np.int64), conformers=rows.conf.astype(np.int64), fit=sm[:, 0].copy(), ideal=sm[:, 1].copy(), fraction=_ratio(sm[:, 0], sm[:, 1]),
                   best_fit=sm[:, 2].copy(), best_ideal=sm[:, 3].copy(), best_fraction=_ratio(sm[:, 2], sm[:, 3]), n_nodes=cn[:, 0].copy(), n_pairs=cn[:, 1].copy(),
                   n_in_place=cn[:, 2].copy(), n_passing=cn[:, 3].copy(), node_fit=cut(nfit, nn), node_best=cut(nbest, nn), node_z2=cut(nz2, nn),
                   node_target=cut(ntgt, nn, np.int64), hotspot_z2=cut(hz2, wm), hotspot_node=cut(hnode, wm, np.int64),
                   occupied_fingerprint=f.host(fp).view(np.uint64).copy(), status=st, device=dev)


# ---------------------------------------------------------------------------------------------------------------- colour: the typed term
@dataclass
class ColourReport:
    """What `colour` returns: one row per posed set of typed points against a known ligand's pharmacophore features (definitions:
    `pmx_pose_colour` in include/pmx.h). Floats are float64. Points and types only - no donor / acceptor direction, no ring normal - and
    first-order overlaps, as the shape term's.

    overlap[i], self_overlap[i], reference_overlap[i]   C_AB, C_AA, C_BB: the weighted Gaussian overlap of the pairs that share a type
    tanimoto[i]     C_AB / (C_AA + C_BB - C_AB), 0 where C_AB is 0: exactly 1 for the reference's own features in place
    reference_fraction[i], fit_fraction[i]   C_AB / C_BB and C_AB / C_AA (0 where the denominator is 0)
    rms_matched[i]  the root mean square, over the nodes that have a partner of a shared weighted type, of the distance to the nearest
                    such feature (NaN where no node has one)
    type_overlap    [n, 7]: the part of C_AB each type carries, in `constants.TYPE_NAMES` order (`by_type(i)` names them); they add up to
                    `overlap` only up to rounding
    n_nodes[i], n_matched[i], n_reference_features[i], n_reference_matched[i]   typed points; those with a typed partner nearer than
                    `cover`; the reference's features; those of them with a typed partner nearer than `cover`
    node_overlap[i], node_distance[i], node_feature[i]   per node its part of C_AB, the distance to its nearest typed partner (NaN
                    without one) and that feature (-1 without one)
    feature_distance[i], feature_node[i]   the mirror image, per reference feature
    matched_fingerprint   uint64 [n, 4]: bit b says reference feature b is reproduced (counted in n_reference_matched); `similarity` and
                    `leaders` cluster hits by which of the binder's interactions they reproduce
    status[i]       0, 1 (PMX_LIGAND_UNSUPPORTED: also a row of more than 64 typed points) or 4 (PMX_LIGAND_KEY_INVALID: not a conformer,
                    a motion that is not finite, a mask >= 128); such a row has NaN, zero counts, -1 and an empty fingerprint"""

    overlap: np.ndarray
    self_overlap: np.ndarray
    reference_overlap: np.ndarray
    tanimoto: np.ndarray
    reference_fraction: np.ndarray
    fit_fraction: np.ndarray
    rms_matched: np.ndarray
    type_overlap: np.ndarray
    n_nodes: np.ndarray
    n_matched: np.ndarray
    n_reference_features: np.ndarray
    n_reference_matched: np.ndarray
    node_overlap: list
    node_distance: list
    node_feature: list
    feature_distance: list
    feature_node: list
    matched_fingerprint: np.ndarray
    status: np.ndarray
    device: "int | None" = None  # where `similarity` and `leaders` run

    def __len__(self) -> int:
        return len(self.status)

    def by_type(self, i: int) -> dict:
        """Row i's `type_overlap`, keyed by type name."""
        from .constants import TYPE_NAMES

        return {name: float(self.type_overlap[i, t]) for t, name in enumerate(TYPE_NAMES)}

    def similarity(self, other: "ColourReport | None" = None) -> np.ndarray:
        """Tanimoto similarity of the matched fingerprints, on the GPU (`fingerprint_similarity`)."""
        return fingerprint_similarity(self.matched_fingerprint, None if other is None else other.matched_fingerprint, device=self.device)

    def leaders(self, threshold: float = 0.7, max_leaders: int = 2048):
        """Sphere exclusion over the rows in their order by matched fingerprint (`fingerprint_leaders`): (leaders, leader_of)."""
        return fingerprint_leaders(self.matched_fingerprint, threshold=threshold, max_leaders=max_leaders, device=self.device)


class _ColourRefHandle(_DeviceHandle):
    _destroy = "pmx_colour_ref_destroy"

    def __init__(self, colour, device: int):
        handle = ctypes.c_void_p()
        xyz, mask = np.ascontiguousarray(colour.xyz, dtype=np.float32), np.ascontiguousarray(colour.typemask, dtype=np.uint8)
        w = (ctypes.c_float * 7)(*[float(v) for v in colour.weights_array()])
        _ffi.check(_ffi.load().pmx_colour_ref_create(xyz.ctypes.data, mask.ctypes.data, len(mask), w, float(colour.radius), device, ctypes.byref(handle)))
        super().__init__(handle, device)
        self.f = len(mask)

    @property
    def self_overlap(self) -> float:
        out = ctypes.c_double()
        _ffi.check(_ffi.load().pmx_colour_ref_self(self.handle, ctypes.byref(out)))
        return out.value


def _colour_of(reference, what: str):
    """The `shape.ColourFeatures` of `reference`: itself, or the `colour` a `shape.ReferenceLigand` carries."""
    from .shape import ColourFeatures

    if isinstance(reference, ColourFeatures):
        return reference
    colour = getattr(reference, "colour", None)
    if colour is None:
        raise ValueError(f"{what}: the reference has no typed features - a shape.ColourFeatures, or a ReferenceLigand with `colour`")
    return colour


def device_colour_ref(reference, device=None) -> _ColourRefHandle:
    """The device copy of a `shape.ColourFeatures` (or of a `ReferenceLigand`'s `colour`), made once per (features, device) and freed with
    the object."""
    colour = _colour_of(reference, "device_colour_ref")
    return _cached_handle(colour._device, _device_index(device), lambda dev: _ColourRefHandle(colour, dev))


def colour(reference, library=None, indices=None, conformers=None, rotation=None, translation=None, features=None, feature_types=None, cover: float = 2.0,
           device=None) -> ColourReport:
    """Posed rows against a known ligand's typed features (`pmx_pose_colour`, csrc/pmx_colour.hip): row i is a set of typed points moved by
    `rotation[i]` and `translation[i]`, `reference` a `shape.ColourFeatures` (or a `ReferenceLigand` that carries one). A pair of a point
    and a feature counts when the two share a type of weight > 0, by the sum of those weights times the Gaussian overlap of two spheres
    of the features' radius. The pose is judged where it is: nothing is moved.
      node mode     `library`, `indices`, `conformers`: the pharmacophore nodes of library ligand indices[i] at conformer conformers[i] with
                    the record's type masks
      feature mode  `features`: a list of [k_i, 3] arrays, typed points of the caller's; `feature_types`: a matching list of type names,
                    ids, or uint8 masks (`shape.type_masks`). A row holds at most 64 (more: status 1); a mask above 127 gives its row status 4
    Exactly one of the two. At most 65536 rows. Runs on torch's current stream of the device and waits for it."""
    from .shape import type_masks

    _torch()
    ref = _colour_of(reference, "colour")
    if (features is None) != (feature_types is None):
        raise ValueError("colour: features and feature_types go together")
    rows = _PoseRows("colour", library, indices, conformers, rotation, translation, features, None)
    masks = None
    if features is not None:
        if len(feature_types) != rows.n:
            raise ValueError(f"{len(feature_types)} lists of types for {rows.n} feature sets")
        each = [type_masks(v, check=False) for v in feature_types]  # (a mask above 127 is the row's status, not an error)
        if any(len(m) != len(np.asarray(p).reshape(-1, 3)) for m, p in zip(each, features)):
            raise ValueError("a list of types differs in length from its features")
        masks = np.ascontiguousarray(np.concatenate(each + [np.zeros(1, np.uint8)]))  # (never an empty buffer)
    if not (np.isfinite(cover) and cover >= 0):
        raise ValueError("cover must be finite and not negative")
    with _pose_frame(rows, library, None, device, device_colour_ref, ref) as f:
        summary, types, count, fp = f.f64(f.m, 8), f.f64(f.m, 7), f.i32(f.m, 4), f.i64(f.m, _FP_WORDS)
        ncol, nnear, nfeat, fnear, fnode = f.f64(f.m, _MAX_NODES), f.f64(f.m, _MAX_NODES), f.i32(f.m, _MAX_NODES), f.f64(f.m, _MAX_NODES), f.i32(f.m, _MAX_NODES)
        t_mask = f.up(masks).data_ptr() if masks is not None else None
        _ffi.check(f.lib.pmx_pose_colour(f.owner.handle, f.library, *f.src[:4], t_mask, *f.motion, f.n, float(cover), summary.data_ptr(), types.data_ptr(), count.data_ptr(),
                                         ncol.data_ptr(), nnear.data_ptr(), nfeat.data_ptr(), fnear.data_ptr(), fnode.data_ptr(), fp.data_ptr(), f.status.data_ptr(), f.stream))
    n, st, nf = f.n, f.st, f.owner.f
    sm, cn = f.host(summary), f.host(count).astype(np.int64)
    nn = np.where(st == 0, cn[:, 0], 0)
    cut = lambda t, k, dtype=None: [(r[: k[i]] if np.ndim(k) else r[:k]).astype(dtype or r.dtype).copy() for i, r in enumerate(f.host(t))]  # noqa: E731
    return ColourReport(overlap=sm[:, 0].copy(), self_overlap=sm[:, 1].copy(), reference_overlap=sm[:, 2].copy(), tanimoto=sm[:, 3].copy(), reference_fraction=sm[:, 4].copy(),
                        fit_fraction=sm[:, 5].copy(), rms_matched=sm[:, 6].copy(), type_overlap=f.host(types).copy(), n_nodes=cn[:, 0].copy(), n_matched=cn[:, 1].copy(),
                        n_reference_matched=cn[:, 2].copy(), n_reference_features=cn[:, 3].copy(), node_overlap=cut(ncol, nn), node_distance=cut(nnear, nn),
                        node_feature=cut(nfeat, nn, np.int64), feature_distance=cut(fnear, nf), feature_node=cut(fnode, nf, np.int64),
                        matched_fingerprint=f.host(fp).view(np.uint64).copy(), status=st, device=f.dev)


@dataclass
class ComboOverlay(ShapeOverlay):
    """What `combo_overlay` returns: a `ShapeOverlay` - every field of it as there, the motion now the one that maximises shape and colour
    together, F = O_AB + colour_weight * C_AB (definitions: `pmx_combo_overlay` in include/pmx.h) - with the colour and combo fields. Rigid
    only, no directions and no hydrogens, first-order overlaps, a local maximum, and `colour_weight` is uncalibrated.

    colour_overlap_start[i], colour_overlap[i]   C_AB at the start motion and at the overlaid one
    colour_self_overlap[i], colour_reference_overlap[i]   C_AA and C_BB
    colour_tanimoto_start[i], colour_tanimoto[i]   C_AB / (C_AA + C_BB - C_AB) before and after, 0 where C_AB is 0
    combo_start[i], combo[i]   the sum of the shape and the colour Tanimoto, 0 to 2 ("TanimotoCombo"), before and after
    n_nodes[i], n_reference_features[i]   the row's typed nodes and the reference's features
    colour_weight   the weight the call ran with
    start, start_tanimoto   with `starts=4`: the start kept is the one of highest final combo, and `start_tanimoto` holds every start's final combo"""

    colour_overlap_start: "np.ndarray | None" = None
    colour_overlap: "np.ndarray | None" = None
    colour_self_overlap: "np.ndarray | None" = None
    colour_reference_overlap: "np.ndarray | None" = None
    colour_tanimoto_start: "np.ndarray | None" = None
    colour_tanimoto: "np.ndarray | None" = None
    combo_start: "np.ndarray | None" = None
    combo: "np.ndarray | None" = None
    n_nodes: "np.ndarray | None" = None
    n_reference_features: "np.ndarray | None" = None
    colour_weight: float = 0.0


def balanced_colour_weight(reference, device=None) -> float:
    """O_BB / C_BB of a `ReferenceLigand` that carries its `colour`: the weight at which the reference laid on itself gets equal amounts
    from the shape and the colour term. A derived default, not a calibrated one; 0 for a reference whose C_BB is 0."""
    o_bb, c_bb = device_shape_ref(reference, device).self_overlap, device_colour_ref(reference, device).self_overlap
    return float(o_bb / c_bb) if c_bb > 0 else 0.0


def combo_overlay(reference, library, indices, conformers, rotation=None, translation=None, atoms=None, colour_weight="balanced", starts: int = 0, node_radius: float = 1.0,
                  ftol: float = 1e-6, max_iter: int = 32, device=None, colour=None, points=None, point_radii=None) -> ComboOverlay:
    """Library rows overlaid on a known ligand by shape and colour together (`pmx_combo_overlay`, csrc/pmx_colour.hip): per row a bounded
    Levenberg-Marquardt maximisation over the rigid motion of F = O_AB + colour_weight * C_AB. `reference` is a `shape.ReferenceLigand`
    that carries its `colour` (`ReferenceLigand.from_library`), or one without and `colour` a `shape.ColourFeatures`. The colour points are
    always the pharmacophore nodes of library ligand indices[i] at conformer conformers[i]; the shape points are those nodes as spheres of
    `node_radius`, or with `atoms` (the library's atom store) the ligand's heavy atoms with Bondi radii, or `points` / `point_radii` of the
    caller's, one set per row. Both move under the one motion.
      colour_weight  "balanced": O_BB / C_BB of the two references (`balanced_colour_weight`) - derived, not calibrated: nobody has
                     measured which weight ranks known binders best. A number: that weight, finite and >= 0; 0 is `overlay`
      starts=0       each row is optimised from its given motion
      starts=4       `rotation` / `translation` are ignored: each hit is run from the four inertial starts of its shape points
                     (`pmx_shape_starts`) and the start of highest final combo is kept, the lower among equals. At most 16384 hits
    Rigid only, no directions, no hydrogens, first-order overlaps, and a local maximum. At most 65536 rows. Runs on torch's current
    stream of the device and waits for it."""
    _torch()
    what = "combo_overlay"
    if library is None:
        raise ValueError(f"{what}: the library is required - the colour points are its records' nodes")
    col = _colour_of(reference if colour is None else colour, what)
    _overlay_check(what, starts, max_iter, ftol, node_radius)
    if not isinstance(colour_weight, str) and not (np.isfinite(colour_weight) and colour_weight >= 0):
        raise ValueError("colour_weight must be finite and not negative, or 'balanced'")
    if isinstance(colour_weight, str) and colour_weight != "balanced":
        raise ValueError("colour_weight: a number, or 'balanced'")
    if atoms is not None and (points is not None or not _is_store(atoms)):
        raise ValueError(f"{what}: atoms is the library's DeviceAtoms / PackedAtoms; points are the alternative to it")
    if point_radii is not None and points is None:
        raise ValueError(f"{what}: point_radii go with points")
    idx, conf = np.asarray(indices).reshape(-1), np.asarray(conformers).reshape(-1)
    idx, conf, rotation, translation, points, point_radii = _expand_starts(what, starts, len(idx), idx, conf, rotation, translation, points, point_radii)
    rows = _PoseRows(what, library, idx, conf, rotation, translation, points, point_radii, atoms, both=True)
    with _pose_frame(rows, library, atoms, device, device_shape_ref, reference) as f:
        chandle = device_colour_ref(col, f.dev)
        cw = (float(f.owner.self_overlap / chandle.self_overlap) if chandle.self_overlap > 0 else 0.0) if isinstance(colour_weight, str) else float(colour_weight)
        rot, trans, energy, count = f.f64(f.m, 3, 3), f.f64(f.m, 3), f.f64(f.m, 16), f.i32(f.m, 6)
        _ffi.check(f.lib.pmx_combo_overlay(f.owner.handle, chandle.handle, f.library, *f.src, *_start_motion(f, starts), f.n, float(node_radius), cw, float(ftol), int(max_iter),
                                           rot.data_ptr(), trans.data_ptr(), energy.data_ptr(), count.data_ptr(), f.status.data_ptr(), f.stream))
    st = f.st
    en, cn, R, t = f.host(energy), f.host(count).astype(np.int64), f.host(rot), f.host(trans)
    pick, start, start_value = _pick_start(en[:, 13], starts)
    return ComboOverlay(rotation=R[pick].copy(), translation=t[pick].copy(), overlap_start=en[pick, 0], overlap=en[pick, 1], self_overlap=en[pick, 2],
                        reference_overlap=en[pick, 3], tanimoto_start=en[pick, 4], tanimoto=en[pick, 5], angle=en[pick, 14], shift=en[pick, 15], iterations=cn[pick, 0],
                        accepted=cn[pick, 1], stop=cn[pick, 2], n_points=cn[pick, 3], start=start, start_tanimoto=start_value, status=st[pick],
                        indices=rows.idx[pick].copy(), conformers=rows.conf[pick].astype(np.int64), colour_overlap_start=en[pick, 6], colour_overlap=en[pick, 7],
                        colour_self_overlap=en[pick, 8], colour_reference_overlap=en[pick, 9], colour_tanimoto_start=en[pick, 10], colour_tanimoto=en[pick, 11],
                        combo_start=en[pick, 12], combo=en[pick, 13], n_nodes=cn[pick, 4], n_reference_features=cn[pick, 5], colour_weight=cw)


def colour_of(poses, reference, library, **kw) -> ColourReport:
    """`colour` of posed rows - an `Alignment`, `RefinedPoses`, `ShapeOverlay` or `ComboOverlay` whose rows are ligands of `library` - at
    their own motions: the rows' pharmacophore nodes compared with a known ligand's typed features. Row i of the report is row i of the
    poses. Further arguments (`cover`) as `colour` takes them. (A function, not a method: the posed classes keep their set of methods.)"""
    if poses.indices is None:
        raise ValueError("colour_of: these rows are points of the caller's, not ligands of a library")
    return colour(reference, library, poses.indices, poses.conformers, poses.rotation, poses.translation, **kw)


def combo_overlay_of(poses, reference, library, atoms=None, **kw) -> ComboOverlay:
    """`combo_overlay` of posed rows from each row's own motion: how far is this pose from its nearest match with a known ligand in shape
    and colour together? The nodes carry the types; the shape points are the nodes or - with `atoms`, the library's atom store - the heavy
    atoms. Further arguments (`colour_weight`, `node_radius`, `ftol`, `max_iter`) as `combo_overlay` takes them."""
    if poses.indices is None:
        raise ValueError("combo_overlay_of: these rows are points of the caller's, not ligands of a library")
    if kw.get("starts", 0):
        raise ValueError("combo_overlay_of: the local overlay of these poses; `combo_overlay(..., starts=4)` is the one that needs no pose")
    return combo_overlay(reference, library, poses.indices, poses.conformers, poses.rotation, poses.translation, atoms=atoms, **kw)
