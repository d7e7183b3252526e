"""CPU emulator of lsf_reinit_band (include/lsf.h), built on the oracle: the yardstick of the band tests.

One band sweep is one full-interior Jacobi sweep of the oracle (lsf_oracle_jacobi_box) followed by
out = where(M, swept, in).  That is exact, not an approximation: a Jacobi update reads only the field as it
was at the start of the sweep, so what the sweep computes for the cells outside M cannot reach the cells inside.
M = the interior points whose mask is 1.  RMS of a sweep = sqrt(sum over M (new - old)^2 / |M|).
"""
import ctypes

import numpy as np

import oracle_lib


def _lib():
    L = oracle_lib.lib()
    i9, i3 = ctypes.c_int * 9, ctypes.c_int * 3
    L.lsf_oracle_jacobi_box.restype = None
    L.lsf_oracle_jacobi_box.argtypes = [ctypes.c_void_p] * 3 + [i9, i3, i3, ctypes.c_double, ctypes.c_double, ctypes.c_void_p]
    return L, i9, i3


def list_mask(mask, nx, ny, nz):
    """Boolean array of the LIST: interior points (1..n-1 in each axis) with mask == 1; any other value is 'out'."""
    m = np.asarray(mask).reshape((nx + 1, ny + 1, nz + 1), order="F") == 1
    inner = np.zeros_like(m)
    inner[1:nx, 1:ny, 1:nz] = True
    return np.asfortranarray(m & inner)


def full_sweep(phi, phiS, nx, ny, nz, dx, h):
    """One oracle Jacobi sweep over the whole interior; wall points of the result hold the input's values."""
    L, i9, i3 = _lib()
    a = np.asfortranarray(phi, dtype=np.float64)
    s = np.asfortranarray(phiS, dtype=np.float64)
    out = a.copy(order="F")
    sumsq = ctypes.c_double(0.0)
    L.lsf_oracle_jacobi_box(a.ctypes.data, out.ctypes.data, s.ctypes.data, i9(nx + 1, ny + 1, nz + 1, 0, 0, 0, nx, ny, nz), i3(1, 1, 1),
                            i3(nx, ny, nz), float(dx), float(h), ctypes.addressof(sumsq))
    return out


def band_sweep(phi, phiS, M, nx, ny, nz, dx, h):
    """Returns (field after one band sweep, RMS of the sweep)."""
    swept = full_sweep(phi, phiS, nx, ny, nz, dx, h)
    out = np.asfortranarray(np.where(M, swept, phi))
    d = (out - phi)[M]
    return out, float(np.sqrt(np.sum(d * d) / d.size))


def reinit_band(phi, mask, nx, ny, nz, iter, dx, h, tol=1e-5, phiS=None):
    """lsf_reinit_band on the CPU.  Returns (field, sweeps done, RMS trace, nan flag); `phi` is not modified."""
    cur = np.array(phi, dtype=np.float64, order="F", copy=True)
    cur = cur.reshape((nx + 1, ny + 1, nz + 1), order="F")
    M = list_mask(mask, nx, ny, nz)
    sgn = cur.copy(order="F") if phiS is None else np.asfortranarray(phiS, dtype=np.float64).reshape(cur.shape, order="F")
    trace = []
    if not M.any():
        return cur, 0, trace, False
    for _ in range(iter + 1):
        cur, rms = band_sweep(cur, sgn, M, nx, ny, nz, dx, h)
        trace.append(rms)
        if rms != rms:
            return cur, len(trace), trace, True
        if rms < tol:
            break
    return cur, len(trace), trace, False
