"""lsf_curvature_band restated in numpy: the serial statement of the contract in include/lsf.h.

    LIST   the interior points with mask == 1 (list_of of tests/advect_band_ref.py); every stencil point of an interior cell lies
           inside the field, so there is one rule for every list cell.
    H, K   mean curvature k1 + k2 = div(grad(phi)/|grad(phi)|) and Gaussian curvature k1 * k2 of the level set through the cell,
           from central second-order differences.

Every expression is evaluated as the header writes it, left to right, on whole arrays (numpy never contracts), so the library's
result is compared with `==`.  The arguments are left alone; an output that is given is written at list cells and nowhere else.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from advect_band_ref import list_of

DEGENERATE_G2 = 1e-24


class CurvResult(NamedTuple):
    kappa: np.ndarray
    gauss: Optional[np.ndarray]
    gmag: Optional[np.ndarray]
    cells: int
    degenerate: int
    clamped: int
    kappa_max: float
    nonfinite: int  # > 0: LSF_ERR_NAN with this count; cells, degenerate, clamped and kappa_max are then not reported


def _s(phi, a, b, c):
    """the neighbour at offset (a, b, c) of every interior cell"""
    n = phi.shape
    return phi[1 + a:n[0] - 1 + a, 1 + b:n[1] - 1 + b, 1 + c:n[2] - 1 + c]


def interior_values(phi, dx, clamp=0.0):
    """(H, K, g, degenerate, clamped_H, clamped_K) on ALL interior cells, arrays of the interior's shape"""
    phi = np.asarray(phi, dtype=np.float64)
    s = lambda a, b, c: _s(phi, a, b, c)
    c = s(0, 0, 0)
    two_dx, dx2 = 2. * dx, dx * dx
    four_dx2 = 4. * dx2
    with np.errstate(all="ignore"):
        px = (s(1, 0, 0) - s(-1, 0, 0)) / two_dx
        py = (s(0, 1, 0) - s(0, -1, 0)) / two_dx
        pz = (s(0, 0, 1) - s(0, 0, -1)) / two_dx
        pxx = ((s(1, 0, 0) - 2. * c) + s(-1, 0, 0)) / dx2
        pyy = ((s(0, 1, 0) - 2. * c) + s(0, -1, 0)) / dx2
        pzz = ((s(0, 0, 1) - 2. * c) + s(0, 0, -1)) / dx2
        pxy = (((s(1, 1, 0) - s(1, -1, 0)) - s(-1, 1, 0)) + s(-1, -1, 0)) / four_dx2
        pxz = (((s(1, 0, 1) - s(1, 0, -1)) - s(-1, 0, 1)) + s(-1, 0, -1)) / four_dx2
        pyz = (((s(0, 1, 1) - s(0, 1, -1)) - s(0, -1, 1)) + s(0, -1, -1)) / four_dx2
        g2 = (px * px + py * py) + pz * pz
        g = np.sqrt(g2)
        num = ((px * px) * (pyy + pzz) + (py * py) * (pxx + pzz)) + (pz * pz) * (pxx + pyy)
        mix = ((px * py) * pxy + (px * pz) * pxz) + (py * pz) * pyz
        H = (num - 2. * mix) / (g2 * g)
        A = ((px * px) * (pyy * pzz - pyz * pyz) + (py * py) * (pxx * pzz - pxz * pxz)) + (pz * pz) * (pxx * pyy - pxy * pxy)
        B = ((px * py) * (pxz * pyz - pxy * pzz) + (py * pz) * (pxy * pxz - pyz * pxx)) + (px * pz) * (pxy * pyz - pxz * pyy)
        K = (A + 2. * B) / (g2 * g2)
        deg = g2 < DEGENERATE_G2  # a NaN g2 is not degenerate
        H = np.where(deg, 0.0, H)
        K = np.where(deg, 0.0, K)
        cH = np.zeros(H.shape, bool)
        cK = np.zeros(H.shape, bool)
        if clamp != 0.0:
            lim = clamp / dx
            lim2 = lim * lim
            cH = (H > lim) | (H < -lim)  # comparisons: a NaN stays NaN
            H = np.where(H > lim, lim, H)
            H = np.where(H < -lim, -lim, H)
            cK = (K > lim2) | (K < -lim2)
            K = np.where(K > lim2, lim2, K)
            K = np.where(K < -lim2, -lim2, K)
    return H, K, g, deg, cH, cK


def curvature_band(phi, mask, dx, kappa, gauss=None, gmag=None, clamp=0.0) -> CurvResult:
    """lsf_curvature_band: returns copies of the outputs given, written at list cells only.  A cell is clamped when a WRITTEN value
    differs from the unclamped one (K counts only where gauss is given); a cell is non-finite when a written value is."""
    lst = list_of(mask)
    outs = [None if a is None else np.array(a, dtype=np.float64, order="F") for a in (kappa, gauss, gmag)]
    if not lst.any():
        return CurvResult(*outs, 0, 0, 0, 0.0, 0)
    I = tuple(slice(1, n - 1) for n in lst.shape)
    L = lst[I]
    H, K, g, deg, cH, cK = interior_values(phi, dx, clamp)
    clamped = cH.copy()
    bad = ~np.isfinite(H)
    outs[0][I][L] = H[L]
    if outs[1] is not None:
        outs[1][I][L] = K[L]
        clamped |= cK
        bad |= ~np.isfinite(K)
    if outs[2] is not None:
        outs[2][I][L] = g[L]
        bad |= ~np.isfinite(g)
    nbad = int(np.count_nonzero(bad & L))
    if nbad:
        return CurvResult(*outs, 0, 0, 0, float("nan"), nbad)
    bits = np.abs(H[L]).view(np.uint64)  # the bit-pattern maximum: no order of reduction in it
    kmax = float(np.array([bits.max()], np.uint64).view(np.float64)[0])
    return CurvResult(*outs, int(L.sum()), int(np.count_nonzero(deg & L)), int(np.count_nonzero(clamped & L)), kmax, 0)
