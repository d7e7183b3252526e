"""The seam of one call: host (numpy arrays; the library copies them to HBM and back) or device (torch CUDA tensors, on the
tensor's current stream).  A wrapper of levelset.py builds one Seam from its arrays, resolves its fields and points through it,
allocates its outputs from it and hands it the C call, written once.  torch is imported on the device seam only.
"""
from __future__ import annotations

import numpy as np

from . import _lib

KINDS = ("numpy arrays", "CUDA tensors")
torch = None  # the module, from the first call on the device seam on
_TORCH_DTYPES = {}  # numpy scalar type -> torch dtype, filled then (np.dtype(t).name would cost 2 us a time)


def _import_torch():
    global torch
    import torch

    _TORCH_DTYPES.update({np.float64: torch.float64, np.float32: torch.float32, np.int32: torch.int32})


def is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


class Seam:
    __slots__ = ("anchor", "dev", "nx", "ny", "nz", "device", "_arrays", "_subject")

    def __init__(self, anchor, nx, ny, nz, subject=None, others=(), optional=(), kinds=KINDS, check_device=True):
        """anchor: the array that decides the seam; others: the call's other arrays, optional: those the caller may leave out (None).
        All must be of the anchor's kind and, for tensors, on its device -- `subject` names them all in the two messages.  A wrapper
        that has always compared the devices later, after its points or fields, says check_device=False and calls one_device()."""
        self.anchor, self.nx, self.ny, self.nz = anchor, nx, ny, nz
        self.dev = dev = type(anchor).__module__.startswith("torch")
        for a in others:  # (plain loops: a wrapper's own time is a few microseconds, and this is most of it)
            if type(a).__module__.startswith("torch") != dev:
                raise TypeError(f"{subject} must all be {kinds[0]} or all be {kinds[1]}")
        for a in optional:
            if a is not None and type(a).__module__.startswith("torch") != dev:
                raise TypeError(f"{subject} must all be {kinds[0]} or all be {kinds[1]}")
        if dev:
            if torch is None:
                _import_torch()
            self.device = anchor.device
            self._arrays, self._subject = (*others, *optional), subject
            if check_device:
                self.one_device()

    def one_device(self):
        """Device seam: every array lives on the anchor's device"""
        if self.dev:
            device = self.device
            for a in self._arrays:
                if a is not None and a.device != device:
                    raise ValueError(f"{self._subject} must live on one device")

    def is_f32(self, a) -> bool:
        """whether `a` is a float32 array of the call's kind (reinit's single-precision path)"""
        if self.dev:
            return a.dtype == torch.float32
        return isinstance(a, np.ndarray) and a.dtype == np.float32

    def field(self, a, name, dtype=np.float64) -> int:
        """The pointer of a field of (nx+1)(ny+1)(nz+1) values: numpy, Fortran-ordered (nx+1, ny+1, nz+1), or a CUDA tensor,
        contiguous (nz+1, ny+1, nx+1); either may be flat"""
        if not self.dev:
            return host_field(a, name, dtype, self.nx, self.ny, self.nz)
        nx, ny, nz, want = self.nx, self.ny, self.nz, _TORCH_DTYPES[dtype]
        if not a.is_cuda or a.dtype != want:
            raise TypeError(f"{name} must be a CUDA tensor of {want}")
        if a.dim() == 3:
            if tuple(a.shape) != (nz + 1, ny + 1, nx + 1):
                raise ValueError(f"{name} must have shape (nz+1, ny+1, nx+1) (i is the unit-stride axis)")
        elif a.dim() != 1 or a.numel() != (nx + 1) * (ny + 1) * (nz + 1):
            raise ValueError(f"{name} must have (nx+1)(ny+1)(nz+1) elements")
        if not a.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        return a.data_ptr()

    def optional(self, a, name, dtype=np.float64):
        """field(), or None for a field the caller left out"""
        return None if a is None else self.field(a, name, dtype)

    def points(self, a, name="pts", count="npts") -> int:
        """n of an (n, 3) float64 array in Fortran order (for a tensor: the transpose of a contiguous (3, n)), the layout of surfX"""
        if len(a.shape) != 2 or a.shape[1] != 3 or a.shape[0] < 1:
            raise ValueError(f"{name} must have shape ({count}, 3) with {count} >= 1")
        if self.dev:
            if not a.is_cuda or a.dtype != torch.float64 or not a.t().is_contiguous():
                raise TypeError(f"{name} must be a float64 CUDA tensor of shape ({count}, 3) in Fortran order (the transpose of a contiguous (3, {count}))")
        elif not isinstance(a, np.ndarray) or a.dtype != np.float64 or not a.flags.f_contiguous:
            raise TypeError(f"{name} must be a Fortran-ordered float64 numpy array of shape ({count}, 3)")
        return int(a.shape[0])

    def vector(self, a, n, name, count="npts") -> None:
        """a contiguous float64 vector of n values, one per point"""
        if tuple(a.shape) != (n,):
            raise ValueError(f"{name} must have shape ({count},)")
        if self.dev:
            if a.dtype != torch.float64 or not a.is_contiguous():
                raise TypeError(f"{name} must be a contiguous float64 CUDA tensor")
        elif not isinstance(a, np.ndarray) or a.dtype != np.float64 or not a.flags.c_contiguous:
            raise TypeError(f"{name} must be a contiguous float64 numpy array")

    def out(self, n, dtype=np.float64):
        """an output of n values in the call's kind"""
        if self.dev:
            return torch.empty(n, dtype=_TORCH_DTYPES[dtype], device=self.device)
        return np.zeros(n, dtype=dtype)

    def out3(self, n, dtype=np.float64):
        """an (n, 3) output in Fortran order in the call's kind"""
        if self.dev:  # the transpose of a contiguous (3, n)
            return torch.empty((3, n), dtype=_TORCH_DTYPES[dtype], device=self.device).t()
        return np.zeros((n, 3), dtype=dtype, order="F")

    def copy3(self, a):
        """a copy of checked points in their own layout"""
        return a.t().clone().t() if self.dev else a.copy(order="F")

    def ptr(self, a):
        """the pointer of an array of the call's kind that needs no check (an output of out(), checked points), or None"""
        if a is None:
            return None
        return a.data_ptr() if self.dev else a.ctypes.data

    def stream(self):
        """Device seam: makes the anchor's device current for the library and returns that device's current stream"""
        index = self.device.index or 0  # (the index, not the torch.device: torch resolves an int at once)
        rc = _lib.load().lsf_set_device(index)
        if rc:
            _lib.check(rc)
        return torch.cuda.current_stream(index).cuda_stream

    def call(self, name, *args) -> int:
        """lib.NAME(*args) on the host seam, lib.NAME_device(*args, stream) on the device seam; returns the library's code"""
        lib = _lib.load()
        if not self.dev:
            return getattr(lib, name)(*args)
        return getattr(lib, name + "_device")(*args, self.stream())


def host_field(a, name, dtype, nx, ny, nz) -> int:
    """The pointer of a numpy field, Fortran-ordered (nx+1, ny+1, nz+1) or flat (Seam.field on the host seam; host-only calls)"""
    if not isinstance(a, np.ndarray) or a.dtype != dtype:
        raise TypeError(f"{name} must be a numpy array of {np.dtype(dtype).name}")
    if a.ndim == 3:
        if a.shape != (nx + 1, ny + 1, nz + 1) or not a.flags.f_contiguous:
            raise ValueError(f"{name} must be Fortran-ordered with shape (nx+1, ny+1, nz+1) = {(nx+1, ny+1, nz+1)}")
    elif a.ndim != 1 or a.size != (nx + 1) * (ny + 1) * (nz + 1) or not a.flags.c_contiguous:
        raise ValueError(f"{name} must have (nx+1)(ny+1)(nz+1) contiguous elements")
    if not a.flags.writeable:
        raise ValueError(f"{name} must be writeable (it is INTENT(INOUT) in the reference)")
    return a.ctypes.data


def xlo(xLo, finite=True):
    """xLo as the three contiguous float64 values the library reads"""
    lo = np.ascontiguousarray(xLo, dtype=np.float64)
    if finite:
        if lo.shape != (3,) or not np.all(np.isfinite(lo)):
            raise ValueError("xLo must hold 3 finite values")
    elif lo.shape != (3,):
        raise ValueError("xLo must hold 3 values")
    return lo


def positive(dx, message="dx must be finite and > 0") -> float:
    dx = float(dx)
    if not (np.isfinite(dx) and dx > 0.0):
        raise ValueError(message)
    return dx


def finite_iso(iso) -> float:
    iso = float(iso)
    if not np.isfinite(iso):
        raise ValueError("iso must be finite")
    return iso


def grid(nx, ny, nz) -> None:
    if min(int(nx), int(ny), int(nz)) < 1:
        raise ValueError("nx, ny, nz must be >= 1")


def named(what, value, table):
    """table[value] for one of the two names of an order, a scheme or an arithmetic"""
    if not isinstance(value, str) or value not in table:
        a, b = table
        raise ValueError(f"{what} must be {a!r} or {b!r}")
    return table[value]
