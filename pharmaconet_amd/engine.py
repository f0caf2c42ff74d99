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
from .atoms import PackedAtoms
from .constants import weights_vector
from .library import PackedLibrary, as_packed_library
from .validation import ENRICH_TILE, FLOAT64_REFUSED, MAX_BOOTSTRAP, MAX_COLUMNS, POISSON1_CDF64, Enrichment, cutoffs_ppm  # noqa: F401  (the table and the tile of include/pmx.h)

__all__ = ["Alignment", "Attribution", "ClashReport", "DeviceAtoms", "DeviceLibrary", "FittingHits", "Enrichment", "Explanation", "LigandFingerprints", "PanelResult", "PoseFit", "ScreeningResult", "SimilarityResult", "align", "attribute", "clashes",
           "enrichment", "explain", "score_one", "screen", "screen_multi", "similar", "sweep", "topk", "device_model", "last_score_stats", "pose_fit", "ShapeReport", "shape",
           "device_shape_ref"]


def _torch():
    import torch

    if not torch.cuda.is_available():
        raise _ffi.PmxError("no GPU visible: pharmaconet_amd scores on an MI355X only (there is no CPU path)")
    return torch


def _device_index(device) -> int:
    torch = _torch()
    if device is None:
        return torch.cuda.current_device()
    dev = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
    return dev.index if dev.index is not None else torch.cuda.current_device()


class _ModelHandle:
    def __init__(self, flat, device: int):
        lib = _ffi.load()
        self.device = device
        self._keep = dict(
            node_type=np.ascontiguousarray(flat.node_type, dtype=np.uint8),
            edge_mean=np.ascontiguousarray(flat.edge_mean, dtype=np.float32),
            edge_std=np.ascontiguousarray(flat.edge_std, dtype=np.float32),
            cluster_nodes=np.ascontiguousarray(flat.cluster_nodes, dtype=np.uint64),
            cluster_typemask=np.ascontiguousarray(flat.cluster_typemask, dtype=np.uint8),
            cluster_center=np.ascontiguousarray(flat.cluster_center, dtype=np.float64),
            cluster_size=np.ascontiguousarray(flat.cluster_size, dtype=np.float64),
        )
        desc = _ffi.ModelDesc(
            flat.num_nodes,
            flat.num_clusters,
            *(self._keep[k].ctypes.data for k in (
                "node_type", "edge_mean", "edge_std", "cluster_nodes", "cluster_typemask", "cluster_center", "cluster_size")),
        )
        handle = ctypes.c_void_p()
        _ffi.check(lib.pmx_model_create(ctypes.byref(desc), device, ctypes.byref(handle)))
        self.handle = handle
        self._node_centers = None
        self._node_sigmas = None

    def node_sigmas(self, model):
        """The model nodes' `radius` as a float64 [Nm] tensor on the handle's device (`pmx_pose_fit`'s sigmas): uploaded on first use, kept."""
        if self._node_sigmas is None:
            torch = _torch()
            host = np.zeros(max(model.num_nodes, 1), dtype=np.float64)  # (never an empty buffer)
            host[: model.num_nodes] = model.node_radii
            self._node_sigmas = torch.from_numpy(host).to(torch.device("cuda", self.device))
        return self._node_sigmas

    def node_centers(self, model):
        """The model nodes' `center` as a float64 [Nm, 3] tensor on the handle's device (`pmx_align`'s targets): uploaded on first use, kept."""
        if self._node_centers is None:
            torch = _torch()
            host = np.zeros((max(model.num_nodes, 1), 3), dtype=np.float64)  # (never an empty buffer: a model without nodes has no pairs either)
            host[: model.num_nodes] = model.node_centers
            self._node_centers = torch.from_numpy(host).to(torch.device("cuda", self.device))
        return self._node_centers

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _ffi.load().pmx_model_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def device_model(model, device=None) -> _ModelHandle:
    """Device tables of a `PharmacophoreModel`, created once per (model, device)."""
    dev = _device_index(device)
    cache = model._engine_handle
    if not isinstance(cache, dict):
        cache = {}
        model._engine_handle = cache
    if dev not in cache:
        cache[dev] = _ModelHandle(model.flat, dev)
    return cache[dev]


class DeviceLibrary:
    """A packed ligand library resident in HBM (upload once, score against many models / weights)."""

    def __init__(self, library: PackedLibrary, device=None):
        self.device = _device_index(device)
        offsets = np.ascontiguousarray(library.offsets, dtype=np.uint64)
        data = np.ascontiguousarray(library.data, dtype=np.uint8)
        self._n_conf = library.headers()[:, 1].copy() if len(library) else np.zeros(0, np.uint16)  # (what `explain` cuts its rows to)
        self._n_nodes = library.headers()[:, 0].copy() if len(library) else np.zeros(0, np.uint16)  # (... and `attribute`)
        view = _ffi.LibraryView(len(library), offsets.ctypes.data, data.ctypes.data if data.size else None, 0)
        self._upload(view)

    def _upload(self, view) -> None:
        """pmx_library_upload of `view` on self.device: the handle and what the library says about itself."""
        lib = _ffi.load()
        handle = ctypes.c_void_p()
        _ffi.check(lib.pmx_library_upload(ctypes.byref(view), self.device, ctypes.byref(handle)))
        self.handle = handle
        info = _ffi.LibraryInfo()
        _ffi.check(lib.pmx_library_info_get(self.handle, ctypes.byref(info)))
        self.num_ligands = int(info.n_ligands)
        self.num_bytes = int(info.n_bytes)
        self.total_conformers = int(info.total_conformers)
        self.max_nodes = int(info.max_nodes)
        self.max_conformers = int(info.max_conformers)
        self.max_clusters = int(info.max_clusters)
        self.num_unsupported = int(info.n_unsupported)

    @classmethod
    def from_device_buffers(cls, offsets, data, device=None, adopt: bool = False) -> "DeviceLibrary":
        """A library already in device memory: `offsets` int64/uint64 [N + 1] and `data` uint8 torch tensors - copied, or with `adopt` used in
        place (the tensors are kept alive by the object and must not be written to while it lives)."""
        torch = _torch()
        self = cls.__new__(cls)
        self.device = _device_index(device if device is not None else offsets.device)
        torch.cuda.current_stream(torch.device("cuda", self.device)).synchronize()  # (pmx_library_upload reads a complete view, on the default stream)
        adopt = adopt and data.numel() > 0  # (an empty library has nothing to adopt: torch hands out a null pointer for it)
        if adopt:
            if not (offsets.is_contiguous() and data.is_contiguous()):
                raise ValueError("adopted buffers must be contiguous")
            self._adopted = (offsets, data)
        view = _ffi.LibraryView(int(offsets.numel()) - 1, offsets.data_ptr(), data.data_ptr(), 2 if adopt else 1)
        self._upload(view)
        return self

    @classmethod
    def from_features(cls, flat, device=None, check: bool = True) -> "DeviceLibrary":
        """Typed features -> resident library without the host packer: `pack_features_device` + adoption of its buffers.
        `flat`: `library.flatten_features(...)` arrays (NumPy: uploaded; or torch tensors already on the device). With `check`
        a molecule outside the device builder's fixed scratch (status 3) raises - pack such a batch with `pack_features_native`."""
        offsets, data, status = pack_features_device(flat, device)
        if check and bool((status == 3).any()):
            raise _ffi.PmxError("a molecule exceeds the device packer's fixed scratch (include/pmx.h): use library.pack_features_native for this batch")
        self = cls.from_device_buffers(offsets, data, device if device is not None else offsets.device, adopt=True)
        self.pack_status = status
        return self

    def __len__(self) -> int:
        return self.num_ligands

    def select(self, indices) -> "DeviceLibrary":
        """The records of ligands `indices` (any order, repeats allowed) as a resident library of their own, gathered on the device
        (`pmx_library_select`, csrc/pmx_select.hip): record i is a byte copy of record `indices[i]`, as `PackedLibrary.select` makes it on
        the host. `indices`: a list, a NumPy array, or an int64 torch tensor on the device (which stays there). Runs on torch's current
        stream; the new library's buffers are torch's, adopted, so `explain`, `attribute`, `align` and `download` work on it. An index outside
        the library is a `PmxError` that says how many there are and where the first is (IndexError for a negative one in a host list)."""
        torch = _torch()
        lib = _ffi.load()
        tdev = torch.device("cuda", self.device)
        idx = _listed_indices(indices, tdev)
        n = int(idx.numel())
        with torch.cuda.device(tdev):
            stream = ctypes.c_void_p(torch.cuda.current_stream(tdev).cuda_stream)
            offsets = torch.empty(n + 1, dtype=torch.int64, device=tdev)
            nbytes = ctypes.c_uint64(0)
            _ffi.check(lib.pmx_library_select(self.handle, idx.data_ptr() if n else None, n, offsets.data_ptr(), None, 0, ctypes.byref(nbytes), stream))
            data = torch.empty(int(nbytes.value), dtype=torch.uint8, device=tdev)
            if data.numel():
                _ffi.check(lib.pmx_library_select(self.handle, idx.data_ptr(), n, offsets.data_ptr(), data.data_ptr(), data.numel(), ctypes.byref(nbytes), stream))
            return DeviceLibrary.from_device_buffers(offsets, data, tdev, adopt=True)  # (waits for the stream: `idx` may go)

    def buffers(self):
        """(offsets int64 [N + 1], data uint8 [bytes]): the device buffers this library reads, as torch tensors - the adopted ones, or views of
        the library's own (`pmx_library_buffers`), valid until `close`. Not to be written to."""
        src = getattr(self, "_adopted", None)
        if src is not None:
            return src
        torch = _torch()
        po, pd = ctypes.c_void_p(), ctypes.c_void_p()
        _ffi.check(_ffi.load().pmx_library_buffers(self.handle, ctypes.byref(po), ctypes.byref(pd)))
        tdev = torch.device("cuda", self.device)

        class _View:  # (torch reads foreign device memory through the CUDA array interface)
            def __init__(self, ptr, count, typestr):
                self.__cuda_array_interface__ = dict(shape=(count,), typestr=typestr, data=(int(ptr), False), version=2, strides=None)

        offsets = torch.as_tensor(_View(po.value, self.num_ligands + 1, "<i8"), device=tdev)
        data = torch.as_tensor(_View(pd.value, self.num_bytes, "|u1"), device=tdev) if self.num_bytes else torch.empty(0, dtype=torch.uint8, device=tdev)
        return offsets, data

    def download(self) -> PackedLibrary:
        """The library as a host `PackedLibrary`, whatever it was made from (waits for torch's current stream)."""
        offsets, data = self.buffers()
        return PackedLibrary(offsets.cpu().numpy().view(np.uint64).copy(), data[: self.num_bytes].cpu().numpy().copy())

    def fingerprints(self, first: int = 0, count: int | None = None, conformers=None) -> "LigandFingerprints":
        """The ligand-side pharmacophore fingerprints and type census of ligands `[first, first + count)` (`pmx_library_fingerprints`,
        csrc/pmx_ligand_fp.hip; the definition is in include/pmx.h). `conformers`: None for the union over a ligand's conformers - what it
        can present - or per ligand a conformer index (a list, a NumPy array or an int32 device tensor; -1 is the union again) - a hit as
        posed. Enqueued on torch's current stream, nothing is read back. The union fingerprints of the whole library are kept on the
        object (32 bytes a ligand) until `close`."""
        torch = _torch()
        whole = first == 0 and count in (None, self.num_ligands) and conformers is None
        if whole and getattr(self, "_fingerprints", None) is not None:
            return self._fingerprints
        count = self.num_ligands - first if count is None else int(count)
        if first < 0 or count < 0 or first + count > self.num_ligands:
            raise IndexError(f"ligands {first} .. {first + count} of a library of {self.num_ligands}")
        tdev = torch.device("cuda", self.device)
        conf = None
        if conformers is not None:
            conf = conformers if isinstance(conformers, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(conformers, dtype=np.int32).reshape(-1)))
            conf = conf.to(tdev).to(torch.int32).reshape(-1).contiguous()
            if int(conf.numel()) != count:
                raise ValueError(f"{int(conf.numel())} conformers for {count} ligands")
        with torch.cuda.device(tdev):
            bits = torch.empty((count, _FP_WORDS), dtype=torch.int64, device=tdev)
            counts = torch.empty((count, 8), dtype=torch.uint8, device=tdev)
            status = torch.empty(count, dtype=torch.int32, device=tdev)
            stream = ctypes.c_void_p(torch.cuda.current_stream(tdev).cuda_stream)
            _ffi.check(_ffi.load().pmx_library_fingerprints(self.handle, first, count, conf.data_ptr() if conf is not None and count else None, bits.data_ptr() if count else None,
                                                            counts.data_ptr() if count else None, status.data_ptr() if count else None, stream))
        out = LigandFingerprints(bits=bits, type_counts=counts, status=status, first=first, device=self.device)
        if whole:
            self._fingerprints = out
        return out

    def where(self, min_counts=None, max_counts=None, max_nodes: int | None = None):
        """The ligands whose type census passes, as an int64 device tensor of library indices, ascending - ready for `select` and
        `screen(indices=...)`. `min_counts` / `max_counts`: per type the least / most nodes that carry it, as a dict keyed by type name
        (`TYPE_NAMES`, as `weights` are given) or a sequence of seven; `max_nodes`: the most nodes. Ligands the fingerprint pass reports
        with a non-zero status (they cannot be scored either) never pass. A few torch operations on `fingerprints().type_counts`."""
        torch = _torch()
        from .constants import TYPE_ID

        fps = self.fingerprints()
        census = fps.type_counts.to(torch.int32)
        keep = fps.status == 0

        def seven(bounds, what):
            if isinstance(bounds, dict):
                unknown = [k for k in bounds if k not in TYPE_ID]
                if unknown:
                    raise ValueError(f"{what}: unknown pharmacophore type {unknown[0]!r}")
                return {TYPE_ID[k]: int(v) for k, v in bounds.items()}
            vals = list(bounds)
            if len(vals) != _ffi.NUM_TYPES:
                raise ValueError(f"{what}: a dict keyed by type name, or seven numbers")
            return {t: int(v) for t, v in enumerate(vals)}

        for t, v in (seven(min_counts, "min_counts") if min_counts is not None else {}).items():
            keep = keep & (census[:, t] >= v)
        for t, v in (seven(max_counts, "max_counts") if max_counts is not None else {}).items():
            keep = keep & (census[:, t] <= v)
        if max_nodes is not None:
            keep = keep & (census[:, 7] <= int(max_nodes))
        return torch.nonzero(keep).reshape(-1)

    def close(self) -> None:
        if getattr(self, "handle", None):
            _ffi.load().pmx_library_destroy(self.handle)
            self.handle = None
        self._adopted = None
        self._fingerprints = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceAtoms:
    """An atom store resident in HBM (`pmx_atoms_upload`, csrc/pmx_atoms.hip): the heavy atoms of every ligand of a library, from which
    `clashes`, `refine` and `pose_search` take a row's points on the device (`atoms=`). The radii are `pocket.atomic_number_radii`'s, copied
    once with the store, so a gathered radius is the bits the list-of-molecules path computes."""

    def __init__(self, atoms: PackedAtoms, device=None):
        from .pocket import atomic_number_radii

        self.device = _device_index(device)
        offsets = np.ascontiguousarray(atoms.offsets, dtype=np.uint64)
        data = np.ascontiguousarray(atoms.data, dtype=np.uint8)
        table = np.ascontiguousarray(atomic_number_radii(np.arange(128)), dtype=np.float32)
        view = _ffi.AtomsView(len(atoms), offsets.ctypes.data, data.ctypes.data if data.size else None)
        lib = _ffi.load()
        handle = ctypes.c_void_p()
        _ffi.check(lib.pmx_atoms_upload(ctypes.byref(view), table.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), self.device, ctypes.byref(handle)))
        self.handle = handle
        info = _ffi.AtomsInfo()
        _ffi.check(lib.pmx_atoms_info_get(self.handle, ctypes.byref(info)))
        self.num_ligands = int(info.n_ligands)
        self.num_bytes = int(info.n_bytes)
        self.max_atoms = int(info.max_atoms)
        self.num_empty = int(info.n_empty)

    def __len__(self) -> int:
        return self.num_ligands

    def gather_device(self, lig, conf, n: int):
        """`pmx_atoms_gather` of rows (lig[i], conf[i]), device tensors (int64, int32) of this store's device, enqueued on torch's current
        stream: (point_off int64 [n + 1], points float32 [cap, 3], radii float32 [cap], status int32 [n]) with cap = max(n * max_atoms, 1)."""
        torch = _torch()
        if self.handle is None:
            raise _ffi.PmxError("this atom store was closed")
        tdev = torch.device("cuda", self.device)
        cap = n * self.max_atoms
        with torch.cuda.device(tdev):
            off = torch.empty(n + 1, dtype=torch.int64, device=tdev)
            points = torch.empty((max(cap, 1), 3), dtype=torch.float32, device=tdev)
            radii = torch.empty(max(cap, 1), dtype=torch.float32, device=tdev)
            status = torch.empty(max(n, 1), dtype=torch.int32, device=tdev)
            stream = torch.cuda.current_stream(tdev)
            _ffi.check(_ffi.load().pmx_atoms_gather(self.handle, lig.data_ptr(), conf.data_ptr(), n, cap, off.data_ptr(), points.data_ptr(), radii.data_ptr(), status.data_ptr(),
                                                    ctypes.c_void_p(stream.cuda_stream)))
        return off, points, radii, status

    def gather(self, indices, conformers):
        """The rows as host arrays, for inspection: (point_off int64 [n + 1], points float32 [total, 3], radii float32 [total], status int32 [n])."""
        torch = _torch()
        idx = np.ascontiguousarray(np.asarray(indices, dtype=np.int64).reshape(-1))
        conf = np.ascontiguousarray(np.clip(np.asarray(conformers, dtype=np.int64).reshape(-1), -1, 2**31 - 1).astype(np.int32))
        if len(idx) != len(conf):
            raise ValueError("indices and conformers differ in length")
        if (idx < 0).any():
            raise ValueError("negative ligand index")
        n = len(idx)
        if n > _ffi.EXPLAIN_MAX:
            raise ValueError("at most 65536 rows per gather (PMX_EXPLAIN_MAX)")
        tdev = torch.device("cuda", self.device)
        lig = torch.from_numpy(idx if n else np.zeros(1, np.int64)).to(tdev)
        cf = torch.from_numpy(conf if n else np.zeros(1, np.int32)).to(tdev)
        off, points, radii, status = self.gather_device(lig, cf, n)
        torch.cuda.current_stream(tdev).synchronize()
        off = off.cpu().numpy()
        total = int(off[-1])
        return off, points.cpu().numpy()[:total].copy(), radii.cpu().numpy()[:total].copy(), status.cpu().numpy()[:n].copy()

    def close(self) -> None:
        if getattr(self, "handle", None):
            _ffi.load().pmx_atoms_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@contextlib.contextmanager
def _resident_atoms(atoms, device: int):
    """A `DeviceAtoms` on `device` for a `DeviceAtoms` (as it is) or a `PackedAtoms` (uploaded for the call and freed after it)."""
    if isinstance(atoms, DeviceAtoms):
        if atoms.device != device:
            raise _ffi.PmxError(f"the atom store is on device {atoms.device}, the call on {device}")
        yield atoms
        return
    dat = DeviceAtoms(atoms, device)
    try:
        yield dat
    finally:
        dat.close()


def _is_store(atoms) -> bool:
    return isinstance(atoms, (DeviceAtoms, PackedAtoms))


def _listed_indices(indices, tdev):
    """A list of ligand indices as a flat int64 tensor on `tdev`: a list or a NumPy array is uploaded, a device tensor stays where it is."""
    torch = _torch()
    if isinstance(indices, torch.Tensor):
        if indices.dtype != torch.int64:
            raise TypeError("ligand indices as a tensor: int64")
        return indices.to(tdev).reshape(-1).contiguous()
    host = np.ascontiguousarray(np.asarray(indices, dtype=np.int64).reshape(-1))
    if (host < 0).any():
        raise IndexError("negative ligand index")
    return torch.from_numpy(host).to(tdev)


@contextlib.contextmanager
def _resident(library, device=None):
    """`library` in HBM for the length of the block: a `DeviceLibrary` as it is, anything else `as_packed_library` accepts uploaded for the
    block and closed behind it, once the device is done with it."""
    if isinstance(library, DeviceLibrary):
        yield library
        return
    owned = DeviceLibrary(as_packed_library(library), device)
    try:
        yield owned
    finally:
        torch = _torch()
        torch.cuda.synchronize(torch.device("cuda", owned.device))
        owned.close()


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
        if conformers not in ("best", "all"):
            raise ValueError("ScreeningResult.overlay: conformers is 'best' or 'all'")
        if starts not in (0, 4):
            raise ValueError("ScreeningResult.overlay: starts is 0 or 4")
        source = (lambda idx, conf: dict(atoms=atoms, indices=idx, conformers=conf)) if atoms is not None else (lambda idx, conf: dict(library=library, indices=idx, conformers=conf))
        if conformers == "best":
            if k * max(starts, 1) > _ffi.EXPLAIN_MAX:
                raise ValueError(f"ScreeningResult.overlay: {k} hits x {max(starts, 1)} starts exceed {_ffi.EXPLAIN_MAX} rows")
            al = explain(model, library, self._best(k), weights=weights).poses(model, library, weights=weights)
            if starts == 0:
                return al.overlay(reference, library if atoms is None else None, atoms=atoms, **kw)
            return overlay(reference, starts=starts, **source(al.indices, al.conformers), **kw)
        if starts == 0:
            raise ValueError("ScreeningResult.overlay: conformers='all' has a fitted pose for one conformer only; use starts=4")
        hits = self._best(k).astype(np.int64)
        with _resident(library) as dlib:
            n_conf = np.maximum(_record_counts(dlib, hits, 1), 1)
        rows = int(n_conf.sum()) * starts
        if rows > _ffi.EXPLAIN_MAX:
            raise ValueError(f"ScreeningResult.overlay: {len(hits)} hits x their conformers x {starts} starts are {rows} rows, more than {_ffi.EXPLAIN_MAX}; lower k or use conformers='best'")
        idx, conf = np.repeat(hits, n_conf), np.concatenate([np.arange(c) for c in n_conf]) if len(hits) else np.zeros(0, np.int64)
        every = overlay(reference, starts=starts, **source(idx, conf), **kw)
        first = np.concatenate([[0], np.cumsum(n_conf)[:-1]]).astype(np.int64) if len(hits) else np.zeros(0, np.int64)
        value = np.where(np.isnan(every.tanimoto), -np.inf, every.tanimoto)
        pick = np.array([lo + int(np.argmax(value[lo: lo + c])) for lo, c in zip(first, n_conf)], dtype=np.int64)  # (the first among equals)
        return ShapeOverlay(**{f.name: (None if getattr(every, f.name) is None else getattr(every, f.name)[pick]) for f in dataclasses.fields(every)})


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
                weights: dict[str, float] | None = None, refine: bool = False, search: int = 0, fit: bool = False, shape=None, **kw) -> "FittingHits":
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
        otherwise; `shape_cover` is its `cover`); nothing else changes."""
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
        passing = np.flatnonzero(rep.ok(max_clashing) & (al.status == 0))[:k]
        return FittingHits(indices=al.indices[passing].astype(np.uint64), scores=ex.scores[al.rows[passing]], ranks=al.rows[passing].astype(np.int64), rows=passing,
                           pool=ex.indices, poses=al, report=rep, refined=refined, fit=pf, shape=sh)

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


def _weights_array(weights):
    return (ctypes.c_float * _ffi.NUM_TYPES)(*weights_vector(weights))


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


NO_MATCH = 0xFF  # include/pmx.h pmx_explain: a level matched to None
NO_LEVEL = 0xFE


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


def _record_counts(library: "DeviceLibrary", idx: np.ndarray, field: int) -> np.ndarray:
    """Header field `field` (0: nodes, 1: conformers) of library ligands `idx` (0 outside the library): kept per ligand when the library was
    uploaded from the host, read from the library's device records (`DeviceLibrary.buffers`) otherwise."""
    ok = idx < len(library)
    j = np.where(ok, idx, 0)
    kept = getattr(library, "_n_conf" if field == 1 else "_n_nodes", None)
    if kept is not None:
        return np.where(ok, kept[j].astype(np.int64) if len(kept) else 0, 0)
    torch = _torch()
    offsets, data = library.buffers()
    starts = offsets.view(torch.int64)[torch.from_numpy(j).to(offsets.device)] + 2 * field
    v = data[starts].to(torch.int64) | (data[starts + 1].to(torch.int64) << 8)
    return np.where(ok, v.cpu().numpy(), 0)


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


_MAX_LEVELS, _MAX_NODES = 20, 64  # PMX_MAX_LEVELS, PMX_MAX_LIGAND_NODES


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


@dataclass
class Alignment:
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
                    of its level); every float of such a row is NaN. A valid row without pairs has R = I, t = 0 and zeros."""

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

    def transform(self, i: int, positions) -> np.ndarray:
        """Row i's motion applied to any [..., 3] array of points of the conformer's frame - a whole molecule's atoms, say: positions @ R.T + t."""
        return np.asarray(positions, dtype=np.float64) @ self.rotation[i].T + self.translation[i]

    def clashes(self, pocket_or_model, library=None, atoms=None, **kw) -> "ClashReport":
        """These poses checked against the pocket's atoms (`clashes`): row i of the report is row i of the alignment, and a row that is
        not OK passes through with status 4. `pocket_or_model`: a `pocket.PocketAtoms`, or a model that carries its protein
        (`PharmacophoreModel.pocket_atoms`). With `library` alone the rows' own pharmacophore nodes are checked (node mode: nothing but the
        resident records is read). With `atoms` - per row the `LigandFeatures` / `Ligand` the record was packed from - the molecule's atoms
        at the row's conformer are, hydrogens left out, with Bondi radii by atomic number (point mode). Further arguments as `clashes` takes them."""
        return _check_poses(self, "Alignment.clashes", pocket_or_model, library, atoms, kw)

    def refine(self, pocket_or_model, library=None, atoms=None, **kw) -> "RefinedPoses":
        """These poses moved out of the pocket's atoms and held near the fit (`refine`): row i of the result is row i of the alignment, and
        a row that is not OK passes through with status 4. With `library` alone the points and the anchors are the rows' pharmacophore
        nodes (node mode); with `atoms` - per row the molecule the record was packed from - they are its heavy atoms with Bondi radii
        (point mode). Further arguments (`restraint`, `max_iter`, `ftol`, `tolerance`, `node_radius`) as `refine` takes them."""
        pocket, source = _pose_source(self, "Alignment.refine", pocket_or_model, library, atoms)
        out = refine(pocket, rotation=self.rotation, translation=self.translation, **source, **kw)
        if out.indices is None:
            out.indices, out.conformers = self.indices.copy(), np.asarray(self.conformers, dtype=np.int64).copy()
        return out

    def pose_fit(self, model, library, keys=None, **kw) -> "PoseFit":
        """How well these poses sit on the model's hotspots (`pose_fit`): row i of the result is row i of the alignment, and a row that
        is not OK passes through with status 4. `keys`: the rows' keys, for the pairs the fit was made on (key mode); None for every pair
        of matching type (free mode). Further arguments (`weights`, `centers`, `sigmas`) as `pose_fit` takes them."""
        return pose_fit(model, library, self.indices, self.conformers, self.rotation, self.translation, keys=keys, **kw)

    def shape(self, reference, library=None, atoms=None, **kw) -> "ShapeReport":
        """These poses compared with a known ligand (`shape`; `reference` a `shape.ReferenceLigand`): row i of the report is row i of the
        alignment, and a row that is not OK passes through with status 4. The points are the rows' pharmacophore nodes with `library`
        alone, the molecules' heavy atoms with `atoms` (per row the molecule, or the library's atom store), as `Alignment.clashes` takes
        them. Further arguments (`node_radius`, `cover`) as `shape` takes them."""
        return _shape_poses(self, "Alignment.shape", reference, library, atoms, kw)

    def overlay(self, reference, library=None, atoms=None, **kw) -> "ShapeOverlay":
        """These poses moved to their nearest shape match with a known ligand (`overlay` from each row's own motion): how far is the fit
        from it, and how much overlap does it lack? Row i of the result is row i of the alignment; the points as `Alignment.shape` takes
        them. Further arguments (`node_radius`, `ftol`, `max_iter`) as `overlay` takes them."""
        return _overlay_poses(self, "Alignment.overlay", reference, library, atoms, kw)


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


class _PocketHandle:
    def __init__(self, pocket, device: int):
        handle = ctypes.c_void_p()
        xyz, radius, group = (np.ascontiguousarray(pocket.xyz, dtype=np.float32), np.ascontiguousarray(pocket.radius, dtype=np.float32),
                              np.ascontiguousarray(pocket.group, dtype=np.uint16))
        n = len(radius)
        _ffi.check(_ffi.load().pmx_pocket_create(xyz.ctypes.data if n else None, radius.ctypes.data if n else None, group.ctypes.data if n else None, n, device,
                                                 ctypes.byref(handle)))
        self.handle, self.device = handle, device

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _ffi.load().pmx_pocket_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def device_pocket(pocket, device=None) -> _PocketHandle:
    """The device copy of a `pocket.PocketAtoms`, made once per (pocket, device) and freed with the object."""
    dev = _device_index(device)
    if dev not in pocket._device:
        pocket._device[dev] = _PocketHandle(pocket, dev)
    return pocket._device[dev]


class _PoseRows:
    """The rows `clashes` and `refine` share: motions and one source of points, checked and laid out as `pmx_pose_clash` and
    `pmx_pose_refine` take them. `what` names the caller in a message."""

    def __init__(self, what, library, indices, conformers, rotation, translation, points, point_radii, atoms=None):
        self.rot = np.ascontiguousarray(np.asarray(rotation, dtype=np.float64).reshape(-1, 3, 3))
        self.trans = np.ascontiguousarray(np.asarray(translation, dtype=np.float64).reshape(-1, 3))
        n = self.n = len(self.rot)
        if len(self.trans) != n:
            raise ValueError("rotation and translation differ in length")
        if n > 65536:
            raise ValueError(f"at most 65536 rows per {what} call (PMX_EXPLAIN_MAX)")
        self.node_mode = library is not None
        self.store = atoms  # a `DeviceAtoms` / `PackedAtoms`: point mode, the points gathered on the device
        if atoms is not None:
            if not _is_store(atoms):
                raise TypeError(f"{what}: atoms is a DeviceAtoms or a PackedAtoms")
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
        else:
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
        """The device tensors (kept alive by the caller) and the seven source and motion arguments that follow the pocket and the library.
        With an atom store (`dat`, resident on `tdev`) the points are gathered there; a row whose gather status is not OK has no points and
        gets a motion of NaN, so that the call reports it as it reports any row that is not OK (`finish` puts the gather's status in)."""
        torch = _torch()
        n = self.n
        up = lambda a: torch.from_numpy(a).to(tdev)  # noqa: E731
        t_rot, t_trans = up(self.rot.reshape(-1, 9) if n else np.zeros((1, 9))), up(self.trans if n else np.zeros((1, 3)))
        if dat is not None:
            t_a, t_b = up(self.idx if n else np.zeros(1, np.int64)), up(self.conf if n else np.zeros(1, np.int32))
            off, pts, rad, self.gstatus = dat.gather_device(t_a, t_b, n)
            if n:
                bad = (self.gstatus != 0)[:, None]
                t_rot, t_trans = t_rot.masked_fill(bad, float("nan")), t_trans.masked_fill(bad, float("nan"))
            self.slots, self._off_dev = max(n * dat.max_atoms, 1), off
            keep, src = (t_rot, t_trans, t_a, t_b, off, pts, rad), (None, None, off.data_ptr(), pts.data_ptr(), rad.data_ptr())
            return keep, src, (t_rot.data_ptr(), t_trans.data_ptr())
        if self.node_mode:
            t_a, t_b = up(self.idx if n else np.zeros(1, np.int64)), up(self.conf if n else np.zeros(1, np.int32))
            keep, src = (t_rot, t_trans, t_a, t_b), (t_a.data_ptr(), t_b.data_ptr(), None, None, None)
        else:
            t_a, t_b, t_c = up(self.off), up(self.flat), (up(self.rad) if self.rad is not None else None)
            keep, src = (t_rot, t_trans, t_a, t_b, t_c), (None, None, t_a.data_ptr(), t_b.data_ptr(), t_c.data_ptr() if t_c is not None else None)
        return keep, src, (t_rot.data_ptr(), t_trans.data_ptr())


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
    torch = _torch()
    lib = _ffi.load()
    rows = _PoseRows("clashes", library, indices, conformers, rotation, translation, points, point_radii, atoms)
    n, node_mode = rows.n, rows.node_mode
    m = max(n, 1)
    with contextlib.ExitStack() as stack:
        dlib = stack.enter_context(_resident(library, device)) if node_mode else None
        dev = dlib.device if node_mode else atoms.device if isinstance(atoms, DeviceAtoms) else _device_index(device)
        dat = stack.enter_context(_resident_atoms(atoms, dev)) if atoms is not None else None
        ph = device_pocket(pocket, dev)
        tdev = torch.device("cuda", dev)
        with torch.cuda.device(tdev):
            keep, src, motion = rows.upload(tdev, dat)
            slots = m * _MAX_NODES if node_mode else rows.slots if dat is not None else max(int(rows.off[-1]), 1)
            summary = torch.empty((m, 4), dtype=torch.float64, device=tdev)
            count = torch.empty((m, 6), dtype=torch.int32, device=tdev)
            ppen = torch.empty(slots, dtype=torch.float64, device=tdev)
            patom = torch.empty(slots, dtype=torch.int32, device=tdev)
            fp = torch.empty((m, _FP_WORDS), dtype=torch.int64, device=tdev)
            status = torch.empty(m, dtype=torch.int32, device=tdev)
            stream = torch.cuda.current_stream(tdev)
            _ffi.check(lib.pmx_pose_clash(ph.handle, dlib.handle if node_mode else None, *src, *motion, n, float(node_radius), float(tolerance), float(contact),
                                          summary.data_ptr(), count.data_ptr(), ppen.data_ptr(), patom.data_ptr(), fp.data_ptr(), status.data_ptr(),
                                          ctypes.c_void_p(stream.cuda_stream)))
            stream.synchronize()
            del keep
        st = rows.finish(status.cpu().numpy()[:n].astype(np.int32))
        if node_mode:
            nn = _record_counts(dlib, rows.idx, 0)
            lo = np.arange(n, dtype=np.int64) * _MAX_NODES
            hi = lo + np.where(st != 1, nn, 0)
        else:
            lo, hi = rows.off[:-1], rows.off[1:]
    sm, cn = summary.cpu().numpy()[:n], count.cpu().numpy()[:n].astype(np.int64)
    pp, pa = ppen.cpu().numpy(), patom.cpu().numpy().astype(np.int64)
    return ClashReport(clearance=sm[:, 0].copy(), overlap=sm[:, 1].copy(), n_points=cn[:, 0].copy(), n_clashing=cn[:, 1].copy(), n_pairs=cn[:, 2].copy(),
                       n_contacts=cn[:, 3].copy(), worst=cn[:, 4:6].copy(), point_penetration=[pp[lo[i]: hi[i]].copy() for i in range(n)],
                       point_atom=[pa[lo[i]: hi[i]].copy() for i in range(n)], contact_fingerprint=fp.cpu().numpy()[:n].view(np.uint64).copy(), status=st, device=dev)


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


class _ShapeRefHandle:
    def __init__(self, reference, device: int):
        handle = ctypes.c_void_p()
        xyz, radius = np.ascontiguousarray(reference.xyz, dtype=np.float32), np.ascontiguousarray(reference.radius, dtype=np.float32)
        _ffi.check(_ffi.load().pmx_shape_ref_create(xyz.ctypes.data, radius.ctypes.data, len(radius), device, ctypes.byref(handle)))
        self.handle, self.device, self.m = handle, device, len(radius)

    @property
    def self_overlap(self) -> float:
        out = ctypes.c_double()
        _ffi.check(_ffi.load().pmx_shape_ref_self(self.handle, ctypes.byref(out)))
        return out.value

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _ffi.load().pmx_shape_ref_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def device_shape_ref(reference, device=None) -> _ShapeRefHandle:
    """The device copy of a `shape.ReferenceLigand`, made once per (reference, device) and freed with the object."""
    dev = _device_index(device)
    if dev not in reference._device:
        reference._device[dev] = _ShapeRefHandle(reference, dev)
    return reference._device[dev]


def shape(reference, library=None, indices=None, conformers=None, rotation=None, translation=None, points=None, point_radii=None, atoms=None,
          node_radius: float = 1.0, cover: float = 2.0, device=None) -> ShapeReport:
    """Posed rows against a known ligand (`pmx_pose_shape`, csrc/pmx_pose_shape.hip): row i is a set of points moved by `rotation[i]` and
    `translation[i]` - what `Alignment` holds - and `reference` a `shape.ReferenceLigand` in the pocket's frame. The Gaussian shape overlap
    of the two, its Tanimoto and Tversky ratios, and nearest-atom distances both ways; a point (a reference atom) is covered when its
    nearest counterpart is closer than `cover`. The pose is judged where it is: nothing is moved. The three sources of points - node mode
    (`library`, `indices`, `conformers`, each node a sphere of `node_radius`), point mode (`points`, `point_radii`) and the atom store
    (`atoms`, `indices`, `conformers`) - are those of `clashes`; a row holds at most 256 points. Exactly one of the three. At most 65536
    rows. Runs on torch's current stream of the device and waits for it."""
    torch = _torch()
    lib = _ffi.load()
    rows = _PoseRows("shape", library, indices, conformers, rotation, translation, points, point_radii, atoms)
    n, node_mode = rows.n, rows.node_mode
    m = max(n, 1)
    with contextlib.ExitStack() as stack:
        dlib = stack.enter_context(_resident(library, device)) if node_mode else None
        dev = dlib.device if node_mode else atoms.device if isinstance(atoms, DeviceAtoms) else _device_index(device)
        dat = stack.enter_context(_resident_atoms(atoms, dev)) if atoms is not None else None
        rh = device_shape_ref(reference, dev)
        tdev = torch.device("cuda", dev)
        with torch.cuda.device(tdev):
            keep, src, motion = rows.upload(tdev, dat)
            slots = m * _MAX_NODES if node_mode else rows.slots if dat is not None else max(int(rows.off[-1]), 1)
            summary = torch.empty((m, 10), dtype=torch.float64, device=tdev)
            count = torch.empty((m, 4), dtype=torch.int32, device=tdev)
            pnear = torch.empty(slots, dtype=torch.float64, device=tdev)
            pref = torch.empty(slots, dtype=torch.int32, device=tdev)
            rnear = torch.empty((m, _ffi.MAX_LIGAND_ATOMS), dtype=torch.float64, device=tdev)
            rpoint = torch.empty((m, _ffi.MAX_LIGAND_ATOMS), dtype=torch.int32, device=tdev)
            status = torch.empty(m, dtype=torch.int32, device=tdev)
            stream = torch.cuda.current_stream(tdev)
            _ffi.check(lib.pmx_pose_shape(rh.handle, dlib.handle if node_mode else None, *src, *motion, n, float(node_radius), float(cover), summary.data_ptr(),
                                          count.data_ptr(), pnear.data_ptr(), pref.data_ptr(), rnear.data_ptr(), rpoint.data_ptr(), status.data_ptr(),
                                          ctypes.c_void_p(stream.cuda_stream)))
            stream.synchronize()
            del keep
        st = rows.finish(status.cpu().numpy()[:n].astype(np.int32))
        if node_mode:
            nn = _record_counts(dlib, rows.idx, 0)
            lo = np.arange(n, dtype=np.int64) * _MAX_NODES
            hi = lo + np.where(st != 1, nn, 0)
        else:
            lo, hi = rows.off[:-1], rows.off[1:]
    sm, cn = summary.cpu().numpy()[:n], count.cpu().numpy()[:n].astype(np.int64)
    pn, pr = pnear.cpu().numpy(), pref.cpu().numpy().astype(np.int64)
    rn, rp = rnear.cpu().numpy()[:n, : rh.m], rpoint.cpu().numpy()[:n, : rh.m].astype(np.int64)
    return ShapeReport(overlap=sm[:, 0].copy(), self_overlap=sm[:, 1].copy(), reference_overlap=sm[:, 2].copy(), tanimoto=sm[:, 3].copy(),
                       reference_fraction=sm[:, 4].copy(), fit_fraction=sm[:, 5].copy(), rms_to_reference=sm[:, 6].copy(), rms_from_reference=sm[:, 7].copy(),
                       rmsd_in_order=sm[:, 8].copy(), n_points=cn[:, 0].copy(), n_covered=cn[:, 1].copy(), n_reference_covered=cn[:, 2].copy(),
                       point_distance=[pn[lo[i]: hi[i]].copy() for i in range(n)], point_reference_atom=[pr[lo[i]: hi[i]].copy() for i in range(n)],
                       reference_distance=[rn[i].copy() for i in range(n)], reference_point=[rp[i].copy() for i in range(n)], status=st)


def _shape_poses(poses, what, reference, library, atoms, kw) -> "ShapeReport":
    _, source = _pose_source(poses, what, None, library, atoms)
    return shape(reference, rotation=poses.rotation, translation=poses.translation, **source, **kw)


@dataclass
class RefinedPoses:
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
    indices, conformers   node mode: the rows' ligands and conformers (None in point mode)"""

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

    def transform(self, i: int, positions) -> np.ndarray:
        """Row i's refined motion applied to any [..., 3] array of points of the conformer's frame: positions @ R.T + t."""
        return np.asarray(positions, dtype=np.float64) @ self.rotation[i].T + self.translation[i]

    def clashes(self, pocket_or_model, library=None, atoms=None, **kw) -> "ClashReport":
        """The refined poses checked against the pocket's atoms, as `Alignment.clashes` checks the fitted ones: the rows' nodes with
        `library`, the molecules' heavy atoms with `atoms`. A row that is not OK passes through with status 4."""
        return _check_poses(self, "RefinedPoses.clashes", pocket_or_model, library, atoms, kw)

    def pose_fit(self, model, library, keys=None, **kw) -> "PoseFit":
        """How well the refined poses sit on the model's hotspots, as `Alignment.pose_fit` says it of the fitted ones (node mode rows
        only: the rows' ligands and conformers). A row the refinement left untouched has the bits it had before."""
        if self.indices is None:
            raise ValueError("RefinedPoses.pose_fit: these rows are points of the caller's, not ligands of a library")
        return pose_fit(model, library, self.indices, self.conformers, self.rotation, self.translation, keys=keys, **kw)

    def shape(self, reference, library=None, atoms=None, **kw) -> "ShapeReport":
        """The refined poses compared with a known ligand, as `Alignment.shape` compares the fitted ones: the rows' nodes with `library`,
        the molecules' heavy atoms with `atoms`. A row that is not OK passes through with status 4."""
        return _shape_poses(self, "RefinedPoses.shape", reference, library, atoms, kw)

    def overlay(self, reference, library=None, atoms=None, **kw) -> "ShapeOverlay":
        """The refined poses moved to their nearest shape match with a known ligand, as `Alignment.overlay` moves the fitted ones."""
        return _overlay_poses(self, "RefinedPoses.overlay", reference, library, atoms, kw)


@dataclass
class ShapeOverlay:
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
    indices, conformers   the rows' ligands and conformers (None for points of the caller's)"""

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

    def transform(self, i: int, positions) -> np.ndarray:
        """Row i's overlaid motion applied to any [..., 3] array of points of the conformer's frame: positions @ R.T + t."""
        return np.asarray(positions, dtype=np.float64) @ self.rotation[i].T + self.translation[i]

    def shape(self, reference, library=None, atoms=None, **kw) -> "ShapeReport":
        """The overlaid poses compared with a known ligand, as `Alignment.shape` compares the fitted ones."""
        return _shape_poses(self, "ShapeOverlay.shape", reference, library, atoms, kw)

    def clashes(self, pocket_or_model, library=None, atoms=None, **kw) -> "ClashReport":
        """The overlaid poses checked against the pocket's atoms, as `Alignment.clashes` checks the fitted ones: a shape overlay knows
        nothing of the protein."""
        return _check_poses(self, "ShapeOverlay.clashes", pocket_or_model, library, atoms, kw)

    def refine(self, pocket_or_model, library=None, atoms=None, **kw) -> "RefinedPoses":
        """The overlaid poses moved out of the pocket's atoms and held near the overlay, as `Alignment.refine` does it of the fitted ones."""
        if self.indices is None:
            raise ValueError("ShapeOverlay.refine: these rows are points of the caller's, not ligands of a library")
        return Alignment.refine(self, pocket_or_model, library, atoms, **kw)

    def pose_fit(self, model, library, keys=None, **kw) -> "PoseFit":
        """How well the overlaid poses sit on the model's hotspots (free mode unless `keys` are given), as `Alignment.pose_fit`."""
        if self.indices is None:
            raise ValueError("ShapeOverlay.pose_fit: these rows are points of the caller's, not ligands of a library")
        return pose_fit(model, library, self.indices, self.conformers, self.rotation, self.translation, keys=keys, **kw)


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
    torch = _torch()
    lib = _ffi.load()
    if starts not in (0, 4):
        raise ValueError("overlay: starts is 0 (from the given motions) or 4 (the inertial starts)")
    if not 0 <= int(max_iter) <= 64:
        raise ValueError("max_iter: 0 to 64 (PMX_REFINE_MAX_ITER)")
    if not (np.isfinite(ftol) and ftol >= 0):
        raise ValueError("ftol must be finite and not negative")
    if not np.isfinite(node_radius):
        raise ValueError("node_radius must be finite")
    k = max(starts, 1)
    if starts:
        hits = len(points) if points is not None else len(np.asarray(indices).reshape(-1))
        if hits > 16384:
            raise ValueError(f"overlay: {hits} hits, at most 16384 with starts=4 (65536 rows)")
        rep = lambda v: None if v is None else [x for x in v for _ in range(k)]  # noqa: E731
        points, point_radii = rep(points), rep(point_radii)
        if indices is not None:
            indices, conformers = np.repeat(np.asarray(indices).reshape(-1), k), np.repeat(np.asarray(conformers).reshape(-1), k)
        rotation, translation = np.zeros((hits * k, 3, 3)), np.zeros((hits * k, 3))
    elif rotation is None or translation is None:
        raise ValueError("overlay: starts=0 optimises the given motions - rotation and translation")
    rows = _PoseRows("overlay", library, indices, conformers, rotation, translation, points, point_radii, atoms)
    n, node_mode = rows.n, rows.node_mode
    m = max(n, 1)
    with contextlib.ExitStack() as stack:
        dlib = stack.enter_context(_resident(library, device)) if node_mode else None
        dev = dlib.device if node_mode else atoms.device if isinstance(atoms, DeviceAtoms) else _device_index(device)
        dat = stack.enter_context(_resident_atoms(atoms, dev)) if atoms is not None else None
        rh = device_shape_ref(reference, dev)
        tdev = torch.device("cuda", dev)
        with torch.cuda.device(tdev):
            keep, src, motion = rows.upload(tdev, dat)
            rot = torch.empty((m, 3, 3), dtype=torch.float64, device=tdev)
            trans = torch.empty((m, 3), dtype=torch.float64, device=tdev)
            energy = torch.empty((m, 8), dtype=torch.float64, device=tdev)
            count = torch.empty((m, 4), dtype=torch.int32, device=tdev)
            status = torch.empty(m, dtype=torch.int32, device=tdev)
            stream = torch.cuda.current_stream(tdev)
            sptr = ctypes.c_void_p(stream.cuda_stream)
            lh = dlib.handle if node_mode else None
            if starts:
                which = torch.arange(m, dtype=torch.int32, device=tdev) % k
                s_rot = torch.empty((m, 9), dtype=torch.float64, device=tdev)
                s_trans = torch.empty((m, 3), dtype=torch.float64, device=tdev)
                frame = torch.empty((m, 16), dtype=torch.float64, device=tdev)
                s_status = torch.empty(m, dtype=torch.int32, device=tdev)
                _ffi.check(lib.pmx_shape_starts(rh.handle, lh, *src[:4], which.data_ptr(), n, s_rot.data_ptr(), s_trans.data_ptr(), frame.data_ptr(), s_status.data_ptr(), sptr))
                if rows.gstatus is not None and n:  # (a row the store has no atoms for stays not OK)
                    bad = (rows.gstatus != 0)[:, None]
                    s_rot, s_trans = s_rot.masked_fill(bad, float("nan")), s_trans.masked_fill(bad, float("nan"))
                keep = (keep, which, s_rot, s_trans, frame, s_status)
                motion = (s_rot.data_ptr(), s_trans.data_ptr())
            _ffi.check(lib.pmx_shape_overlay(rh.handle, lh, *src, *motion, n, float(node_radius), float(ftol), int(max_iter), rot.data_ptr(), trans.data_ptr(),
                                             energy.data_ptr(), count.data_ptr(), status.data_ptr(), sptr))
            stream.synchronize()
            del keep
    st = rows.finish(status.cpu().numpy()[:n].astype(np.int32))
    en, cn = energy.cpu().numpy()[:n], count.cpu().numpy()[:n].astype(np.int64)
    R, t = rot.cpu().numpy()[:n], trans.cpu().numpy()[:n]
    hits = n // k
    if starts:
        each = en[:, 5].reshape(hits, k)
        best = np.argmax(np.where(np.isnan(each), -np.inf, each), axis=1) if hits else np.zeros(0, np.int64)  # (the first among equals)
        pick = np.arange(hits) * k + best
        start, start_tanimoto = best.astype(np.int64), each.copy()
    else:
        pick, start, start_tanimoto = np.arange(n), np.full(n, -1, np.int64), np.zeros((n, 0))
    has_rows = node_mode or atoms is not None
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


def overlay_starts(reference, start, library=None, indices=None, conformers=None, points=None, atoms=None, device=None) -> ShapeStarts:
    """The inertial start motions of rows (`pmx_shape_starts`): row i's points - as `overlay` takes them - laid with their unweighted
    inertial frame on the reference's, start[i] = 0, or 1 .. 3 for a further half turn about the row's first, second or third axis. What
    `overlay(..., starts=4)` runs from. At most 65536 rows."""
    torch = _torch()
    lib = _ffi.load()
    start = np.ascontiguousarray(np.clip(np.asarray(start, dtype=np.int64).reshape(-1), -1, 2**31 - 1).astype(np.int32))
    n = len(start)
    rows = _PoseRows("overlay_starts", library, indices, conformers, np.zeros((n, 3, 3)), np.zeros((n, 3)), points, None, atoms)
    node_mode = rows.node_mode
    m = max(n, 1)
    with contextlib.ExitStack() as stack:
        dlib = stack.enter_context(_resident(library, device)) if node_mode else None
        dev = dlib.device if node_mode else atoms.device if isinstance(atoms, DeviceAtoms) else _device_index(device)
        dat = stack.enter_context(_resident_atoms(atoms, dev)) if atoms is not None else None
        rh = device_shape_ref(reference, dev)
        tdev = torch.device("cuda", dev)
        with torch.cuda.device(tdev):
            keep, src, _ = rows.upload(tdev, dat)
            which = torch.from_numpy(start if n else np.zeros(1, np.int32)).to(tdev)
            rot = torch.empty((m, 3, 3), dtype=torch.float64, device=tdev)
            trans = torch.empty((m, 3), dtype=torch.float64, device=tdev)
            frame = torch.empty((m, 16), dtype=torch.float64, device=tdev)
            status = torch.empty(m, dtype=torch.int32, device=tdev)
            stream = torch.cuda.current_stream(tdev)
            _ffi.check(lib.pmx_shape_starts(rh.handle, dlib.handle if node_mode else None, *src[:4], which.data_ptr(), n, rot.data_ptr(), trans.data_ptr(), frame.data_ptr(),
                                            status.data_ptr(), ctypes.c_void_p(stream.cuda_stream)))
            stream.synchronize()
            del keep
    st = rows.finish(status.cpu().numpy()[:n].astype(np.int32))
    R, t, fr = rot.cpu().numpy()[:n].copy(), trans.cpu().numpy()[:n].copy(), frame.cpu().numpy()[:n].copy()
    if rows.gstatus is not None:  # (a row the store has no atoms for is not OK, whatever its empty point list gave)
        for a in (R, t, fr):
            a[st != 0] = np.nan
    return ShapeStarts(rotation=R, translation=t, centre=fr[:, 0:3].copy(), axes=fr[:, 3:12].reshape(-1, 3, 3).copy(), values=fr[:, 12:15].copy(), status=st)


def _overlay_poses(poses, what, reference, library, atoms, kw) -> "ShapeOverlay":
    if kw.get("starts", 0):
        raise ValueError(f"{what}: the local overlay of these poses; `overlay(..., starts=4)` is the one that needs no pose")
    _, source = _pose_source(poses, what, None, library, atoms)
    out = overlay(reference, rotation=poses.rotation, translation=poses.translation, **source, **kw)
    if out.indices is None and poses.indices is not None:
        out.indices, out.conformers = np.asarray(poses.indices).copy(), np.asarray(poses.conformers, dtype=np.int64).copy()
    return out


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


def _check_poses(poses, what, pocket_or_model, library, atoms, kw) -> "ClashReport":
    pocket, source = _pose_source(poses, what, pocket_or_model, library, atoms)
    return clashes(pocket, rotation=poses.rotation, translation=poses.translation, **source, **kw)


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
    torch = _torch()
    lib = _ffi.load()
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
    m = max(n, 1)
    with contextlib.ExitStack() as stack:
        dlib = stack.enter_context(_resident(library, device)) if node_mode else None
        dev = dlib.device if node_mode else atoms.device if isinstance(atoms, DeviceAtoms) else _device_index(device)
        dat = stack.enter_context(_resident_atoms(atoms, dev)) if atoms is not None else None
        ph = device_pocket(pocket, dev)
        tdev = torch.device("cuda", dev)
        with torch.cuda.device(tdev):
            keep, src, motion = rows.upload(tdev, dat)
            t_anchor = [None if a is None else torch.from_numpy(a).to(tdev) for a in (a_off, a_flat, a_tgt, a_wts)]
            rot = torch.empty((m, 3, 3), dtype=torch.float64, device=tdev)
            trans = torch.empty((m, 3), dtype=torch.float64, device=tdev)
            energy = torch.empty((m, 8), dtype=torch.float64, device=tdev)
            count = torch.empty((m, 4), dtype=torch.int32, device=tdev)
            status = torch.empty(m, dtype=torch.int32, device=tdev)
            stream = torch.cuda.current_stream(tdev)
            _ffi.check(lib.pmx_pose_refine(ph.handle, dlib.handle if node_mode else None, *src, *(None if a is None else a.data_ptr() for a in t_anchor), *motion, n,
                                           float(node_radius), float(tolerance), float(restraint), float(ftol), int(max_iter), rot.data_ptr(), trans.data_ptr(),
                                           energy.data_ptr(), count.data_ptr(), status.data_ptr(), ctypes.c_void_p(stream.cuda_stream)))
            stream.synchronize()
            del keep, t_anchor
    en, cn = energy.cpu().numpy()[:n], count.cpu().numpy()[:n].astype(np.int64)
    return RefinedPoses(rotation=rot.cpu().numpy()[:n].copy(), translation=trans.cpu().numpy()[:n].copy(), overlap_start=en[:, 0].copy(), overlap=en[:, 2].copy(),
                        restraint_start=en[:, 1].copy(), restraint_energy=en[:, 3].copy(), anchor_rmsd=en[:, 4].copy(), angle=en[:, 5].copy(), shift=en[:, 6].copy(),
                        iterations=cn[:, 0].copy(), accepted=cn[:, 1].copy(), stop=cn[:, 2].copy(), n_pairs=cn[:, 3].copy(),
                        status=rows.finish(status.cpu().numpy()[:n].astype(np.int32)), indices=rows.idx.copy() if node_mode else None,
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
    torch = _torch()
    lib = _ffi.load()
    rows = _PoseRows("pose_fit", library, indices, conformers, rotation, translation, None, None)
    n = rows.n
    nm = int(model.num_nodes)
    kb = None
    if keys is not None:
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
    m = max(n, 1)
    with _resident(library, device) as dlib:
        mh = device_model(model, dlib.device)
        dev = dlib.device
        tdev = torch.device("cuda", dev)
        with torch.cuda.device(tdev):
            keep, src, motion = rows.upload(tdev)
            t_cen = mh.node_centers(model) if over[0] is None else torch.from_numpy(over[0]).to(tdev)
            t_sig = mh.node_sigmas(model) if over[1] is None else torch.from_numpy(over[1]).to(tdev)
            t_key = None if kb is None else torch.from_numpy(kb).to(tdev)
            f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=tdev)  # noqa: E731
            i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=tdev)  # noqa: E731
            summary, count = f64(m, 4), i32(m, 4)
            nfit, nbest, nz2, ntgt = f64(m, _MAX_NODES), f64(m, _MAX_NODES), f64(m, _MAX_NODES), i32(m, _MAX_NODES)
            hz2, hnode = f64(m, _MAX_MODEL_NODES), i32(m, _MAX_MODEL_NODES)
            fp = torch.empty((m, _FP_WORDS), dtype=torch.int64, device=tdev)
            status = i32(m)
            stream = torch.cuda.current_stream(tdev)
            _ffi.check(lib.pmx_pose_fit(mh.handle, dlib.handle, _weights_array(weights), t_cen.data_ptr(), t_sig.data_ptr(), src[0], src[1],
                                        None if t_key is None else t_key.data_ptr(), *motion, n, summary.data_ptr(), count.data_ptr(), nfit.data_ptr(), nbest.data_ptr(),
                                        nz2.data_ptr(), ntgt.data_ptr(), hz2.data_ptr(), hnode.data_ptr(), fp.data_ptr(), status.data_ptr(), ctypes.c_void_p(stream.cuda_stream)))
            stream.synchronize()
            del keep, t_key
        st = status.cpu().numpy()[:n].astype(np.int32)
        nn = np.where(st != 1, _record_counts(dlib, rows.idx, 0), 0) if n else np.zeros(0, np.int64)
    sm, cn = summary.cpu().numpy()[:n], count.cpu().numpy()[:n].astype(np.int64)
    cut = lambda t, w, dt=None: [(a[: w[i]].copy() if dt is None else a[: w[i]].astype(dt)) for i, a in enumerate(t.cpu().numpy()[:n])]  # noqa: E731
    wm = np.full(n, nm, dtype=np.int64)
    return PoseFit(indices=rows.idx.astype(np.int64), conformers=rows.conf.astype(np.int64), fit=sm[:, 0].copy(), ideal=sm[:, 1].copy(), fraction=_ratio(sm[:, 0], sm[:, 1]),
                   best_fit=sm[:, 2].copy(), best_ideal=sm[:, 3].copy(), best_fraction=_ratio(sm[:, 2], sm[:, 3]), n_nodes=cn[:, 0].copy(), n_pairs=cn[:, 1].copy(),
                   n_in_place=cn[:, 2].copy(), n_passing=cn[:, 3].copy(), node_fit=cut(nfit, nn), node_best=cut(nbest, nn), node_z2=cut(nz2, nn),
                   node_target=cut(ntgt, nn, np.int64), hotspot_z2=cut(hz2, wm), hotspot_node=cut(hnode, wm, np.int64),
                   occupied_fingerprint=fp.cpu().numpy()[:n].view(np.uint64).copy(), status=st, device=dev)


_MAX_MODEL_NODES, _FP_WORDS, _MAX_LEADERS = 256, 4, 2048  # PMX_MAX_MODEL_NODES, PMX_FINGERPRINT_WORDS, PMX_MAX_LEADERS
_MAX_QUERIES = 64  # PMX_SEARCH_MAX_QUERIES


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
