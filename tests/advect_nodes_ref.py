"""lsf_advect_nodes restated in numpy: firstDeriv order 8 on a mask (subs.f90:303-358, set3d.f90:470-479) and the per-node move
loop with setPhiSurf's trilinear interpolation (subs.f90:1056-1170, set3d.f90:485-501), on whole arrays.

Every expression is evaluated as the reference writes it, left to right (numpy never contracts), so the result is compared with
`==` against the oracle (tests/test_advect_nodes_cpu.py), which is pinned to the reference itself.  Kept from the reference:
  * neighbours are addressed LINEARLY, as Fortran does without bounds checking: a cell fewer than 4 points from an x or y wall reads
    the neighbouring row / plane;
  * a read before the first or after the last element of phi (undefined in the reference) yields 0 (include/lsf.h);
  * the y derivative uses phi(i,j+1,k) twice (subs.f90:346);
  * a direction with squared length < 1e-7 is zeroed, and a node moves while phiSurf > 1e-13.
A node's value depends on its own position alone, so the reference's loop (which re-interpolates every node after every single move)
is the per-node loop written here.

`defect=` switches ONE deliberate error on.  The defects exist to show that the inputs of tests/advect_nodes_inputs.py discriminate:
each must change the result on the input set named for it in DEFECTS.  They live in this numpy code only (gathers are clipped into the
arrays, so a wrong index reads a wrong element, never outside); no defect is ever applied to a kernel.
"""
from __future__ import annotations

import numpy as np

from advect_nodes_inputs import STRIDE_LIMIT

# defect -> the input set (tests/advect_nodes_inputs.py) that must expose it
DEFECTS = {
    "plane_stride_squared": "cells-13x11x9-ones",   # (nx+1)(ny+1) written as (nx+1)^2
    "extents_swapped": "cells-13x11x9-ones",        # ny and nz exchanged
    "lo_swapped": "cells-13x11x9-ones",             # xLo[1] and xLo[2] exchanged
    "jp2": "cells-13x11x9-ones",                    # phi(i,j+2,k) where the reference repeats phi(i,j+1,k)
    "xd_yd_swapped": "cells-13x11x9-ones",          # interpolation weights of x and y exchanged
    "mask_nonzero": "cells-13x11x9-bernoulli",      # band test `!= 0` instead of `== 1`
    "clamp_reads": "cells-3x3x3-ones",              # out-of-allocation reads clamped to the nearest element instead of 0
    "ge_threshold": "threshold-13x11x9",            # `>=` in the 1e-13 test
    "one_pass_more": "synth-post-1",                # iters + 1 passes
    "grad_first_trip_only": "sphere-131x127x140",   # gradient of the first 2 097 152 points only, zero beyond
}


def _extents(nx, ny, nz, defect):
    """(sx, sxy, n) as the code under the defect would compute them"""
    if defect == "extents_swapped":
        ny, nz = nz, ny
    sx = nx + 1
    sxy = sx * sx if defect == "plane_stride_squared" else sx * (ny + 1)
    return sx, sxy, sxy * (nz + 1)


def firstderiv8(phi, phiSB, nx, ny, nz, dx, defect=None):
    """gradPhi (0:nx,0:ny,0:nz,3), Fortran-ordered: the order-8 derivatives where phiSB == 1, zero elsewhere."""
    assert phi.shape == (nx + 1, ny + 1, nz + 1) and phiSB.shape == phi.shape
    f = np.ascontiguousarray(phi.ravel(order="F"), dtype=np.float64)
    m = np.ascontiguousarray(phiSB.ravel(order="F"))
    size = f.size
    sx, sxy, n = _extents(nx, ny, nz, defect)
    p = np.arange(size, dtype=np.int64)

    def L(off):
        q = p + off
        v = f[np.clip(q, 0, size - 1)]
        if defect == "clamp_reads":
            return v
        return np.where((q < 0) | (q >= n), 0.0, v)

    aa1, aa2, aa3, aa4, aa6, aa7, aa8, aa9 = 1. / 280., -4. / 105., 1. / 5., -4. / 5., 4. / 5, -1. / 5., 4. / 105., -1. / 280.
    jp = 2 * sx if defect == "jp2" else sx  # subs.f90:346
    with np.errstate(invalid="ignore", over="ignore"):
        gx = (L(-4) * aa1 + L(-3) * aa2 + L(-2) * aa3 + L(-1) * aa4 + L(1) * aa6 + L(2) * aa7 + L(3) * aa8 + L(4) * aa9) / dx
        gy = (L(-4 * sx) * aa1 + L(-3 * sx) * aa2 + L(-2 * sx) * aa3 + L(-sx) * aa4 + L(sx) * aa6 + L(jp) * aa7 + L(3 * sx) * aa8
              + L(4 * sx) * aa9) / dx
        gz = (L(-4 * sxy) * aa1 + L(-3 * sxy) * aa2 + L(-2 * sxy) * aa3 + L(-sxy) * aa4 + L(sxy) * aa6 + L(2 * sxy) * aa7
              + L(3 * sxy) * aa8 + L(4 * sxy) * aa9) / dx
    band = (m != 0) if defect == "mask_nonzero" else (m == 1)
    if defect == "grad_first_trip_only":
        band = band & (p < STRIDE_LIMIT)
    grad = np.zeros((size, 3), order="F")
    for c, g in enumerate((gx, gy, gz)):
        grad[:, c] = np.where(band, g, 0.0)
    return grad.reshape(phi.shape + (3,), order="F")


def _interp(f, g3, sx, sxy, dx, lo, X, defect):
    """setPhiSurf for the node rows X: (phiSurf, gradPhiSurf)"""
    size = f.size
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    i0 = np.floor((x - lo[0]) / dx).astype(np.int64)
    j0 = np.floor((y - lo[1]) / dx).astype(np.int64)
    k0 = np.floor((z - lo[2]) / dx).astype(np.int64)
    x0, y0, z0 = i0 * dx + lo[0], j0 * dx + lo[1], k0 * dx + lo[2]
    x1, y1, z1 = (i0 + 1) * dx + lo[0], (j0 + 1) * dx + lo[1], (k0 + 1) * dx + lo[2]
    xd, yd, zd = (x - x0) / (x1 - x0), (y - y0) / (y1 - y0), (z - z0) / (z1 - z0)
    if defect == "xd_yd_swapped":
        xd, yd = yd, xd
    p = i0 + sx * j0 + sxy * k0
    at = lambda a, off: a[np.clip(p + off, 0, size - 1)]
    out = []
    for a in (f, g3[:, 0], g3[:, 1], g3[:, 2]):
        c00 = at(a, 0) * (1. - xd) + at(a, 1) * xd
        c10 = at(a, sx) * (1. - xd) + at(a, sx + 1) * xd
        c01 = at(a, sxy) * (1. - xd) + at(a, sxy + 1) * xd
        c11 = at(a, sxy + sx) * (1. - xd) + at(a, sxy + sx + 1) * xd
        c0 = c00 * (1. - yd) + c10 * yd
        c1 = c01 * (1. - yd) + c11 * yd
        out.append(c0 * (1. - zd) + c1 * zd)
    g = np.stack([-out[1], -out[2], -out[3]], axis=1)
    m2 = g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2]
    small = m2 < 1.E-7
    mag = np.sqrt(np.where(small, 1.0, m2))
    g = np.where(small[:, None], 0.0, g / mag[:, None])
    return out[0], g


def advect(phi, gradPhi, nx, ny, nz, dx, xLo, surfX, iters=1000, defect=None):
    """The move loop of set3d.f90:485-501 on the rows of surfX; returns the advected nodes (nSurfNode,3), Fortran-ordered."""
    f = np.ascontiguousarray(phi.ravel(order="F"), dtype=np.float64)
    g3 = gradPhi.reshape((f.size, 3), order="F")
    sx, sxy, _ = _extents(nx, ny, nz, defect)
    lo = [float(v) for v in xLo]
    if defect == "lo_swapped":
        lo[1], lo[2] = lo[2], lo[1]
    X = np.array(surfX, dtype=np.float64, order="C", copy=True)
    if defect == "one_pass_more":
        iters = iters + 1
    live = np.arange(X.shape[0])
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ps, g = _interp(f, g3, sx, sxy, dx, lo, X, defect)
        for _ in range(iters):
            go = (ps >= 1E-13) if defect == "ge_threshold" else (ps > 1E-13)
            live, ps, g = live[go], ps[go], g[go]
            if live.size == 0:
                break  # nothing moves any more: every later pass repeats this test
            for c in range(3):
                X[live, c] = X[live, c] + ps * g[:, c]
            ps, g = _interp(f, g3, sx, sxy, dx, lo, X[live], defect)
    return np.asfortranarray(X)


def advect_nodes(phi, phiSB, nx, ny, nz, dx, xLo, surfX, iters=1000, defect=None):
    """lsf_advect_nodes: gradients on the cells of phiSB, then the move loop."""
    grad = firstderiv8(phi, phiSB, nx, ny, nz, dx, defect=defect)
    return advect(phi, grad, nx, ny, nz, dx, xLo, surfX, iters=iters, defect=defect)


def narrowband(phi, dx):
    """narrowBand (subs.f90:178-207): (phiNB, phiSB) as int32, same layout as phi."""
    with np.errstate(invalid="ignore"):
        a = np.abs(phi)
        return (a < 4.1 * dx).astype(np.int32, order="F"), (a < 8.1 * dx).astype(np.int32, order="F")
