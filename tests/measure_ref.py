"""lsf_measure_band restated in Python: the serial statement of the contract in include/lsf.h.

    LIST      the interior points with mask == 1 (list_of of tests/advect_band_ref.py)
    MEASURED  a cell of lsf_extract_surface, named by its lower corner c0, whose c0 is in LIST; its seven other corners are read from
              the field whether they are list points or not
    surface   f = phi - iso, inside means f < 0; the six Kuhn tetrahedra, the nodes and the triangles of tests/extract_ref.py
              (tet_offsets, tet_triangles): the triangles measured are, one for one, those lsf_extract_surface emits for the cell

One loop over the crossed measured cells in ascending linear index of c0; inside it Python floats (IEEE binary64, one rounding per
operation, never contracted) in the header's evaluation order, so the library's cell_area is compared with `==` and its totals
against math.fsum of the per-cell contributions.  The arguments are left alone.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np

from advect_band_ref import list_of
from extract_ref import TET_NEGATIVE, tet_offsets, tet_triangles

NQ = 9  # area, volume, x dV, y dV, z dV, x dS, y dS, z dS, q dS
# the 19 edges of the six tetrahedra of a cell: corner offsets u < v (x + 2y + 4z) with the bits of u among those of v
KUHN_EDGES = tuple((u, v) for v in range(8) for u in range(v) if u & v == u)
# per tetrahedron and inside pattern the triangles as corner-offset pairs
_TRIS = [[[[(tet_offsets(t)[u], tet_offsets(t)[v]) for u, v in tri] for tri in tet_triangles(code, TET_NEGATIVE[t])] for code in range(16)]
         for t in range(6)]


class Invalid(ValueError):
    """What the library refuses with LSF_ERR_INVALID; .count = the number the message carries (0: none)."""

    def __init__(self, msg, count=0):
        super().__init__(msg)
        self.count = count


class MeasureResult(NamedTuple):
    cell_area: Optional[np.ndarray]  # a copy of the array given, written at list points only; None when none was given
    cells_c0: np.ndarray             # (crossed, 3) the lower corners of the crossed measured cells, ascending linear index
    contrib: np.ndarray              # (crossed, 9) their contributions to the nine quantities
    M: tuple                         # the nine totals, math.fsum of the columns of contrib
    abs_sum: tuple                   # math.fsum of |contrib| per column: the scale of the summation bound
    cells: int                       # info[0] list cells
    crossed: int                     # info[1] crossed measured cells
    triangles: int                   # info[2]
    open: int                        # info[3] crossed cells with a face-neighbour cell outside LIST
    degenerate: int                  # info[4] triangles with a == 0.0

    @property
    def info(self):
        return [self.cells, self.crossed, self.triangles, self.open, self.degenerate]


def triangle_terms(P0, P1, P2, q0=0.0, q1=0.0, q2=0.0):
    """The nine terms of one triangle, as the header writes them.  P: (x, y, z) of a vertex."""
    e1 = (P1[0] - P0[0], P1[1] - P0[1], P1[2] - P0[2])
    e2 = (P2[0] - P0[0], P2[1] - P0[1], P2[2] - P0[2])
    n = (e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0])
    a = 0.5 * math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    c = (P1[1] * P2[2] - P1[2] * P2[1], P1[2] * P2[0] - P1[0] * P2[2], P1[0] * P2[1] - P1[1] * P2[0])
    v = ((P0[0] * c[0] + P0[1] * c[1]) + P0[2] * c[2]) / 6.0
    m, s = [], []
    for A in range(3):
        s01, s12, s20 = P0[A] + P1[A], P1[A] + P2[A], P2[A] + P0[A]
        m.append((n[A] * ((s01 * s01 + s12 * s12) + s20 * s20)) / 48.0)
        s.append(a * (((P0[A] + P1[A]) + P2[A]) / 3.0))
    qa = a * (((q0 + q1) + q2) / 3.0)
    return (a, v, m[0], m[1], m[2], s[0], s[1], s[2], qa)


def measure_band(phi, mask, dx, xLo, iso=0.0, q=None, cell_area=None) -> MeasureResult:
    """lsf_measure_band.  phi, q, cell_area: (nx+1, ny+1, nz+1) float64; mask: the same shape, int32.  Raises Invalid as the library
    refuses.  The totals are math.fsum over the cells: the library's differ by its own (fixed) order of summation."""
    phi = np.asarray(phi, dtype=np.float64)
    shape = phi.shape
    if min(shape) < 3:
        raise Invalid("nx, ny, nz must be >= 2")
    dx, iso = float(dx), float(iso)
    lo = [float(v) for v in xLo]
    if not (math.isfinite(dx) and dx > 0.0):
        raise Invalid("dx must be finite and > 0")
    if not math.isfinite(iso):
        raise Invalid("iso must be finite")
    if len(lo) != 3 or not all(math.isfinite(v) for v in lo):
        raise Invalid("xLo must hold three finite values")
    for name, a in (("mask", mask), ("q", q), ("cell_area", cell_area)):
        if a is not None and np.shape(a) != shape:
            raise Invalid(f"{name} must have phi's shape")
    if cell_area is not None and (np.shares_memory(cell_area, phi) or (q is not None and np.shares_memory(cell_area, q))):
        raise Invalid("cell_area overlaps an input")
    lst = list_of(np.asarray(mask))
    with np.errstate(invalid="ignore", over="ignore"):
        f = phi - np.float64(iso)
    inside = f < 0
    # the corner byte of every cell, 0 where c0 is not in LIST (an interior c0 has all eight corners in the field)
    cs = tuple(slice(0, n - 1) for n in shape)
    byte = np.zeros(tuple(n - 1 for n in shape), dtype=np.int64)
    for o in range(8):
        byte |= inside[tuple(slice(o >> A & 1, shape[A] - 1 + (o >> A & 1)) for A in range(3))].astype(np.int64) << o
    crossed = (byte != 0) & (byte != 255) & lst[cs]
    idx = np.argwhere(crossed)
    if len(idx):
        idx = idx[np.argsort(idx[:, 0] + shape[0] * (idx[:, 1] + shape[1] * idx[:, 2]), kind="stable")]
    corner = lambda c0, o: (c0[0] + (o & 1), c0[1] + (o >> 1 & 1), c0[2] + (o >> 2 & 1))

    # ---- validation: crossed edges of measured cells with a non-finite endpoint, counted once per measured cell that holds them
    fin_f = np.isfinite(f)
    fin_q = np.isfinite(q) if q is not None else None
    bad_f = bad_q = 0
    for c0 in idx:
        for u, v in KUHN_EDGES:
            a, b = corner(c0, u), corner(c0, v)
            if inside[a] != inside[b]:
                bad_f += not (fin_f[a] and fin_f[b])
                if q is not None:
                    bad_q += not (fin_q[a] and fin_q[b])
    if bad_f:
        raise Invalid(f"{bad_f} crossed edge(s) of measured cells with a non-finite phi - iso on an endpoint", bad_f)
    if bad_q:
        raise Invalid(f"{bad_q} crossed edge(s) of measured cells with a non-finite q on an endpoint", bad_q)

    # ---- the measured cells
    out = None if cell_area is None else np.array(cell_area, dtype=np.float64, order="F")
    if out is not None:
        out[lst] = 0.0
    contrib = np.zeros((len(idx), NQ), dtype=np.float64)
    ntri = ndeg = nopen = 0
    for row, c0 in enumerate(idx):
        c0 = tuple(int(v) for v in c0)
        nodes = {}

        def node(u, v):
            if (u, v) not in nodes:
                a, b = corner(c0, u), corner(c0, v)
                fa, fb = float(f[a]), float(f[b])
                t = fa / (fa - fb)
                d = u ^ v
                X = tuple(lo[A] + (float(a[A]) + t) * dx if d >> A & 1 else lo[A] + float(a[A]) * dx for A in range(3))
                qn = 0.0
                if q is not None:
                    qa, qb = float(q[a]), float(q[b])
                    qn = qa + t * (qb - qa)
                nodes[(u, v)] = (X, qn)
            return nodes[(u, v)]

        acc = [0.0] * NQ
        bt = int(byte[c0])
        for t in range(6):
            offs = tet_offsets(t)
            code = sum((bt >> offs[m] & 1) << m for m in range(4))
            for tri in _TRIS[t][code]:
                (P0, q0), (P1, q1), (P2, q2) = (node(u, v) for u, v in tri)
                terms = triangle_terms(P0, P1, P2, q0, q1, q2)
                for k in range(NQ):
                    acc[k] = acc[k] + terms[k]
                ntri += 1
                ndeg += terms[0] == 0.0
        contrib[row] = acc
        if out is not None:
            out[c0] = acc[0]
        # OPEN: a face-neighbour cell c0 +- e_A whose lower corner is not in LIST (a wall point never is)
        nopen += not all(lst[tuple(c0[B] + (s if B == A else 0) for B in range(3))] for A in range(3) for s in (-1, 1))
    M = tuple(math.fsum(contrib[:, k]) for k in range(NQ))
    S = tuple(math.fsum(np.abs(contrib[:, k])) for k in range(NQ))
    return MeasureResult(out, idx, contrib, M, S, int(lst.sum()), len(idx), ntri, nopen, ndeg)


def summation_bound(res: MeasureResult, k: int) -> float:
    """The largest distance between ANY order of summation of column k and its exact sum: (N - 1) u sum|x| / (1 - (N - 1) u) <= N u
    sum|x| for N u < 1 (Higham, Accuracy and Stability of Numerical Algorithms, (4.4)), u = 2^-53, N the crossed measured cells.
    Adding the exact zeros of the uncrossed cells is exact and does not enter."""
    return res.crossed * 2.0 ** -53 * res.abs_sum[k]


def mesh_measures(X, E):
    """(area, signed volume, surface centroid) of an indexed mesh (1-based E) with fsum: what a caller computes today from
    lsf_extract_surface + lsf_extract_get"""
    X = np.asarray(X, dtype=np.float64)
    E = np.asarray(E, dtype=np.int64) - 1
    terms = [triangle_terms(tuple(X[a]), tuple(X[b]), tuple(X[c])) for a, b, c in E]
    T = np.array(terms).reshape(-1, NQ)
    tot = [math.fsum(T[:, k]) for k in range(NQ)]
    return tot[0], tot[1], tuple(tot[5 + A] / tot[0] for A in range(3)) if tot[0] else (0.0, 0.0, 0.0)
