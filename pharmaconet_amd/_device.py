"""Residency: what lives on the device between calls - the resident library and atom store, the device handles of models, pockets and
reference ligands - and the small helpers every layer above takes the device from. `engine.py` and `poses.py` build on this module."""

from __future__ import annotations

import contextlib
import ctypes

import numpy as np

from . import _ffi
from .atoms import PackedAtoms
from .constants import weights_vector
from .library import PackedLibrary, as_packed_library

NO_MATCH = 0xFF  # include/pmx.h pmx_explain: a level matched to None
NO_LEVEL = 0xFE
_MAX_LEVELS, _MAX_NODES = 20, 64  # PMX_MAX_LEVELS, PMX_MAX_LIGAND_NODES
_MAX_MODEL_NODES, _FP_WORDS, _MAX_LEADERS = 256, 4, 2048  # PMX_MAX_MODEL_NODES, PMX_FINGERPRINT_WORDS, PMX_MAX_LEADERS
_MAX_QUERIES = 64  # PMX_SEARCH_MAX_QUERIES


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


class _DeviceHandle:
    """A device object of libpmx and its lifecycle: `handle` and `device`, and the `_ffi` function named by `_destroy`, called once when the
    object goes."""

    _destroy = None

    def __init__(self, handle, device: int):
        self.handle, self.device = handle, device

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                getattr(_ffi.load(), self._destroy)(self.handle)
                self.handle = None
        except Exception:
            pass


def _cached_handle(cache: dict, dev: int, make):
    """`cache[dev]`, made by `make(dev)` the first time: one device object per (owner, device), freed with the owner."""
    if dev not in cache:
        cache[dev] = make(dev)
    return cache[dev]


class _ModelHandle(_DeviceHandle):
    _destroy = "pmx_model_destroy"

    def __init__(self, flat, device: int):
        lib = _ffi.load()
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
        super().__init__(handle, device)
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


def device_model(model, device=None) -> _ModelHandle:
    """Device tables of a `PharmacophoreModel`, created once per (model, device)."""
    if not isinstance(model._engine_handle, dict):
        model._engine_handle = {}
    return _cached_handle(model._engine_handle, _device_index(device), lambda dev: _ModelHandle(model.flat, dev))


def _weights_array(weights):
    return (ctypes.c_float * _ffi.NUM_TYPES)(*weights_vector(weights))


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
        from .engine import pack_features_device

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
        from .engine import LigandFingerprints

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
