"""lsf_cut_cells_band restated in Python: the serial statement of the contract in include/lsf.h.

    LIST      the interior points with mask == 1 (list_of of tests/advect_band_ref.py); a list point c0 names the cell whose lower
              corner it is, and the seven other corners are read from the field whether they are listed or not
    surface   f = phi - iso, inside means f < 0; the six Kuhn tetrahedra, the nodes and the triangles of tests/extract_ref.py, in
              CELL UNITS: c0 at the origin, dx = 1, so a node is (bit_A(u) + (t if the edge runs along A else 0)) per axis
    per cell  the lower-face apertures, the surface's area vector and the volume fraction by the divergence theorem about c0

One loop over the cut cells in ascending linear index of c0; inside it Python floats (IEEE binary64, one rounding per operation, never
contracted) in the header's evaluation order, so every per-cell output of the library is compared with `==` and its volume against
math.fsum of the stored fractions.  The arguments are left alone.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np

from advect_band_ref import list_of
from extract_ref import tet_offsets
from measure_ref import _TRIS, KUHN_EDGES, Invalid, triangle_terms

U = 2.0 ** -53
CAP = 64 * U  # a cell: at most 18 triangles with a handful of roundings each, on magnitudes <= 1


# ---------------------------------------------------------------------------------- one cell from its eight f values
def edge_fraction(f, m, j):
    """s(m, j): the fraction of the edge from corner m to the zero crossing on the edge {m, j} -- the node's own t when m is the
    edge's lower endpoint, 1.0 - t otherwise"""
    u, v = (m, j) if m < j else (j, m)
    t = f[u] / (f[u] - f[v])
    return t if m == u else 1.0 - t


def tri_fraction(f, a, b, c):
    """the inside fraction of the face triangle (a, b, c) with linear f"""
    ins = [m for m in (a, b, c) if f[m] < 0.0]
    out = [m for m in (a, b, c) if not f[m] < 0.0]
    if not ins:
        return 0.0
    if not out:
        return 1.0
    if len(ins) == 1:
        return edge_fraction(f, ins[0], out[0]) * edge_fraction(f, ins[0], out[1])
    return 1.0 - edge_fraction(f, out[0], ins[0]) * edge_fraction(f, out[0], ins[1])


def face_aperture(f, A, base):
    """the aperture of the face normal to axis A at base in {0, 1 << A}, cut along the Kuhn diagonal base - base|b|c"""
    B, C = (x for x in range(3) if x != A)
    b, c = 1 << B, 1 << C
    return 0.5 * (tri_fraction(f, base, base | b, base | b | c) + tri_fraction(f, base, base | c, base | b | c))


def node(f, u, v):
    """the node on the edge between the corner offsets u < v, in cell units"""
    t = f[u] / (f[u] - f[v])
    d = u ^ v
    return tuple(float(u >> A & 1) + t if d >> A & 1 else float(u >> A & 1) for A in range(3))


class Cell(NamedTuple):
    byte: int
    low: tuple   # face(A, 0): what ax, ay, az hold
    up: tuple    # face(A, 1 << A)
    b: tuple     # sum of 0.5 * n over the triangles
    V: float     # sum of P0 . (P1 x P2) / 6
    raw: float   # ((up_x + up_y) + up_z) / 3.0 + V
    vof: float   # raw clamped to [0, 1]
    clamped: bool
    triangles: int


def cell(f) -> Cell:
    """one cell from f at its eight corners (offset x + 2y + 4z), any corner byte"""
    f = [float(v) for v in f]
    byte = sum((1 << o) for o in range(8) if f[o] < 0.0)
    if byte == 0:
        return Cell(0, (0.0,) * 3, (0.0,) * 3, (0.0,) * 3, 0.0, 0.0, 0.0, False, 0)
    if byte == 255:
        return Cell(255, (1.0,) * 3, (1.0,) * 3, (0.0,) * 3, 0.0, 1.0, 1.0, False, 0)
    V, b, ntri = 0.0, [0.0, 0.0, 0.0], 0
    for t in range(6):
        offs = tet_offsets(t)
        code = sum((byte >> offs[m] & 1) << m for m in range(4))
        for tri in _TRIS[t][code]:
            P0, P1, P2 = (node(f, u, v) for u, v in tri)
            e1 = (P1[0] - P0[0], P1[1] - P0[1], P1[2] - P0[2])
            e2 = (P2[0] - P0[0], P2[1] - P0[1], P2[2] - P0[2])
            n = (e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0])
            for A in range(3):
                b[A] = b[A] + 0.5 * n[A]
            V = V + triangle_terms(P0, P1, P2)[1]
            ntri += 1
    low = tuple(face_aperture(f, A, 0) for A in range(3))
    up = tuple(face_aperture(f, A, 1 << A) for A in range(3))
    raw = ((up[0] + up[1]) + up[2]) / 3.0 + V
    vof = 0.0 if raw < 0.0 else (1.0 if raw > 1.0 else raw)
    return Cell(byte, low, up, tuple(b), V, raw, vof, raw < 0.0 or raw > 1.0, ntri)


def tetrahedra_fraction(f):
    """the volume fraction of a cell by closed forms per Kuhn tetrahedron, independent of the triangles: one inside vertex m the
    product of its three edge fractions, three inside 1 - the product about the outside one, two inside p, q and two outside r, s
    s_pr s_ps + s_pr (1 - s_ps) s_qs + (1 - s_pr) s_qr s_qs; a cell is a sixth of the sum"""
    f = [float(v) for v in f]
    tot = 0.0
    for t in range(6):
        offs = tet_offsets(t)
        ins = [o for o in offs if f[o] < 0.0]
        out = [o for o in offs if not f[o] < 0.0]
        s = lambda m, j: edge_fraction(f, m, j)
        if len(ins) == 4:
            tot += 1.0
        elif len(ins) == 1:
            tot += s(ins[0], out[0]) * s(ins[0], out[1]) * s(ins[0], out[2])
        elif len(ins) == 3:
            tot += 1.0 - s(out[0], ins[0]) * s(out[0], ins[1]) * s(out[0], ins[2])
        elif len(ins) == 2:
            (p, q), (r, z) = ins, out
            tot += s(p, r) * s(p, z) + s(p, r) * (1.0 - s(p, z)) * s(q, z) + (1.0 - s(p, r)) * s(q, r) * s(q, z)
    return tot / 6.0


# ---------------------------------------------------------------------------------- the call
class CutResult(NamedTuple):
    vof: Optional[np.ndarray]         # copies of the arrays given, written at list points only; None where none was given
    aperture: Optional[tuple]         # (ax, ay, az)
    area_vector: Optional[tuple]      # (bx, by, bz)
    cells_c0: np.ndarray              # (cut, 3) the lower corners of the cut cells, ascending linear index
    cut_cells: list                   # their Cell records
    stored: np.ndarray                # the stored vof of every list cell, ascending linear index
    volume: float                     # math.fsum(stored) * ((dx * dx) * dx)
    abs_sum: float                    # math.fsum(|stored|): the scale of the summation bound
    vof_min: float                    # the smallest stored vof over the cut cells, +inf without one
    cells: int                        # info[0] list cells
    cut: int                          # info[1] cut cells
    full: int                         # info[2] full cells
    open: int                         # info[3] cut cells with a face-neighbour cell outside LIST
    clamped: int                      # info[4] cut cells whose raw was clamped

    @property
    def info(self):
        return [self.cells, self.cut, self.full, self.open, self.clamped]


def corner_bytes(f, shape):
    """the corner byte of every cell (lower corners 0 .. n-2 on each axis)"""
    inside = f < 0
    byte = np.zeros(tuple(n - 1 for n in shape), dtype=np.int64)
    for o in range(8):
        byte |= inside[tuple(slice(o >> A & 1, shape[A] - 1 + (o >> A & 1)) for A in range(3))].astype(np.int64) << o
    return byte


def cut_cells_band(phi, mask, dx, iso=0.0, vof=None, aperture=None, area_vector=None) -> CutResult:
    """lsf_cut_cells_band.  phi and the outputs: (nx+1, ny+1, nz+1) float64; mask: the same shape, int32.  Raises Invalid as the
    library refuses.  volume is math.fsum over the list cells: the library's differs by its own (fixed) order of summation."""
    phi = np.asarray(phi, dtype=np.float64)
    shape = phi.shape
    if min(shape) < 3:
        raise Invalid("nx, ny, nz must be >= 2")
    dx, iso = float(dx), float(iso)
    if not (math.isfinite(dx) and dx > 0.0):
        raise Invalid("dx must be finite and > 0")
    if not math.isfinite(iso):
        raise Invalid("iso must be finite")
    outs = [("vof", vof)]
    for name, g in (("aperture", aperture), ("area_vector", area_vector)):
        if g is not None and (len(g) != 3 or any(a is None for a in g)):
            raise Invalid(f"{name} is given whole or not at all")
        outs += [(f"{name}[{A}]", None if g is None else g[A]) for A in range(3)]
    given = [(n, a) for n, a in outs if a is not None]
    for n, a in given + [("mask", mask)]:
        if np.shape(a) != shape:
            raise Invalid(f"{n} must have phi's shape")
    for q, (n, a) in enumerate(given):
        if np.shares_memory(a, phi) or np.shares_memory(a, mask) or any(np.shares_memory(a, o) for _, o in given[:q]):
            raise Invalid(f"{n} overlaps another array")
    lst = list_of(np.asarray(mask))
    with np.errstate(invalid="ignore", over="ignore"):
        f = phi - np.float64(iso)
    cs = tuple(slice(0, n - 1) for n in shape)
    byte = corner_bytes(f, shape)
    listed = lst[cs]
    lin = lambda idx: idx[:, 0] + shape[0] * (idx[:, 1] + shape[1] * idx[:, 2])
    idx = np.argwhere((byte != 0) & (byte != 255) & listed)
    if len(idx):
        idx = idx[np.argsort(lin(idx), kind="stable")]
    corner = lambda c0, o: (c0[0] + (o & 1), c0[1] + (o >> 1 & 1), c0[2] + (o >> 2 & 1))

    # ---- validation: the rule of lsf_measure_band
    fin = np.isfinite(f)
    inside = f < 0
    bad = 0
    for c0 in idx:
        for u, v in KUHN_EDGES:
            a, b = corner(c0, u), corner(c0, v)
            if inside[a] != inside[b]:
                bad += not (fin[a] and fin[b])
    if bad:
        raise Invalid(f"{bad} crossed edge(s) of listed cells with a non-finite phi - iso on an endpoint", bad)

    # ---- the cells
    copy = lambda a: None if a is None else np.array(a, dtype=np.float64, order="F")
    o_vof = copy(vof)
    o_a = None if aperture is None else tuple(copy(a) for a in aperture)
    o_b = None if area_vector is None else tuple(copy(a) for a in area_vector)
    full = np.zeros(shape, bool)
    full[cs] = (byte == 255) & listed
    stored = np.zeros(shape, dtype=np.float64, order="F")
    stored[full] = 1.0
    if o_vof is not None:
        o_vof[lst] = 0.0
        o_vof[full] = 1.0
    for A in range(3):
        if o_a is not None:
            o_a[A][lst] = 0.0
            o_a[A][full] = 1.0
        if o_b is not None:
            o_b[A][lst] = 0.0
    cells, nopen, nclamp = [], 0, 0
    for c0 in idx:
        c0 = tuple(int(v) for v in c0)
        c = cell([f[corner(c0, o)] for o in range(8)])
        cells.append(c)
        stored[c0] = c.vof
        nclamp += c.clamped
        if o_vof is not None:
            o_vof[c0] = c.vof
        for A in range(3):
            if o_a is not None:
                o_a[A][c0] = c.low[A]
            if o_b is not None:
                o_b[A][c0] = c.b[A]
        nopen += not all(lst[tuple(c0[B] + (s if B == A else 0) for B in range(3))] for A in range(3) for s in (-1, 1))
    per_list = stored[lst]  # (boolean indexing of an F-ordered array walks it in C order; fsum does not care)
    vmin = min((c.vof for c in cells), default=math.inf)
    return CutResult(o_vof, o_a, o_b, idx, cells, per_list, math.fsum(per_list) * ((dx * dx) * dx), math.fsum(np.abs(per_list)), vmin,
                     int(lst.sum()), len(idx), int(full.sum()), nopen, nclamp)


def volume_bound(res: CutResult, volume, dx) -> float:
    """How far the library's volume may lie from res.volume: any order of summation of the N non-zero stored fractions is within
    N u sum|x| of their exact sum (Higham (4.4); the zeros add exactly), which the factor (dx dx) dx scales; the product itself rounds
    once in the library and once here."""
    n = int(np.count_nonzero(res.stored))
    d3 = (dx * dx) * dx
    return n * U * res.abs_sum * d3 + U * (abs(volume) + abs(res.volume))
