"""The contract of lsf_extract_surface (include/lsf.h) restated in numpy: marching tetrahedra on the six Kuhn tetrahedra of every
cell, one node per crossed edge, the same numbering and the same arithmetic operation by operation, so that the GPU tests compare
nodes, connectivity, counts and info with ==.  Serial in meaning, vectorised in form: about 10^6 points take seconds.

Conventions (all of them are the header's):
  point      (i,j,k), 0 <= i <= nx ..., linear index p = i + (nx+1)*(j + (ny+1)*k); a cell is named by its lower corner
  inside     f = phi - iso < 0; anything else (+0, -0, NaN) is outside
  edge type  e = dx + 2*dy + 4*dz - 1 for the edge from a to a + (dx,dy,dz): 0 x, 1 y, 2 xy, 3 z, 4 xz, 5 yz, 6 xyz
  node       key 7*p + e, numbered from 1 in ascending key; t = fa / (fa - fb) from the lower endpoint a
  tetrahedra 0..5 = axis orders xyz, xzy, yxz, yzx, zxy, zyx; vertices v0 = c0, v1 = v0 + e_A, v2 = v1 + e_B, v3 = v2 + e_C;
             parity + for 0, 3, 4 (even permutations), - for 1, 2, 5
"""
import numpy as np

AXIS_ORDERS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
TET_NEGATIVE = (False, True, True, False, False, True)
POPCOUNT = np.array([bin(v).count("1") for v in range(256)], dtype=np.int64)


class NonFinite(ValueError):
    """A crossed edge has a non-finite endpoint; .count = the number of such edges (LSF_ERR_INVALID in the library)."""

    def __init__(self, count):
        super().__init__(f"{count} crossed edge(s) with a non-finite endpoint")
        self.count = count


def tet_offsets(t):
    """Corner offsets (as bits x + 2y + 4z) of the four vertices of tetrahedron t."""
    A, B, C = AXIS_ORDERS[t]
    return (0, 1 << A, (1 << A) | (1 << B), 7)


def tet_triangles(code, negative):
    """The triangles of a tetrahedron whose vertex m is inside where bit m of `code` is set: a list of triangles, each a list of
    three edges (u, v), u < v, vertex indices 0..3.  The header's rule:
      one vertex m alone on its side (1 or 3 inside), the others a < b < c:  (ma, mb, mc), the last two swapped when
          flip = negative xor (m odd) xor (3 inside)
      two inside p < q, two outside r < s: (pr, ps, qs) and (pr, qs, qr) -- the quad pr, ps, qs, qr cut along pr-qs --, the last two
          of each swapped when flip = negative xor (p + q even)."""
    ins = [m for m in range(4) if code >> m & 1]
    out = [m for m in range(4) if not code >> m & 1]
    E = lambda u, v: (min(u, v), max(u, v))
    if len(ins) in (0, 4):
        return []
    if len(ins) == 2:
        (p, q), (r, s) = ins, out
        flip = negative ^ ((p + q) % 2 == 0)
        tris = [[E(p, r), E(p, s), E(q, s)], [E(p, r), E(q, s), E(q, r)]]
    else:
        m = ins[0] if len(ins) == 1 else out[0]
        a, b, c = [v for v in range(4) if v != m]
        flip = negative ^ (m % 2 == 1) ^ (len(ins) == 3)
        tris = [[E(m, a), E(m, b), E(m, c)]]
    return [[tr[0], tr[2], tr[1]] if flip else tr for tr in tris]


def extract(phi, dx, xLo, iso=0.0):
    """phi: (nx+1, ny+1, nz+1) float64.  Returns (surfX (nNode,3) float64, surfElem (nTri,3) int32 1-based, info[4]):
    info = nodes, triangles, cells crossed, nodes with t == 1.  Raises NonFinite as the library refuses."""
    phi = np.asarray(phi, dtype=np.float64)
    NX, NY, NZ = phi.shape
    dx = np.float64(dx)
    lo = np.asarray(xLo, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        f = phi - np.float64(iso)
    inside = f < 0
    lin = (np.arange(NX)[:, None, None] + NX * (np.arange(NY)[None, :, None] + NY * np.arange(NZ)[None, None, :])).astype(np.int64)
    shape = (NX, NY, NZ)

    def lower(d):  # the block of points a for which a + d exists, and that of the points a + d
        sa = tuple(slice(0, shape[A] - (d >> A & 1)) for A in range(3))
        sb = tuple(slice(d >> A & 1, shape[A]) for A in range(3))
        return sa, sb

    # ---- nodes: the crossed-edge mask of every point, offsets in linear order
    mask = np.zeros(shape, dtype=np.int64)
    bad = 0
    for e in range(7):
        sa, sb = lower(e + 1)
        crossed = inside[sa] != inside[sb]
        mask[sa] |= crossed.astype(np.int64) << e
        bad += int((crossed & ~(np.isfinite(f[sa]) & np.isfinite(f[sb]))).sum())
    if bad:
        raise NonFinite(bad)
    mflat = mask.ravel(order="F")
    cnt = POPCOUNT[mflat]
    off = np.concatenate(([0], np.cumsum(cnt)))  # off[p] = nodes before point p
    nn = int(off[-1])
    X = np.zeros((nn, 3), dtype=np.float64, order="F")
    n_t1 = 0
    idx = np.indices(shape)
    for e in range(7):
        d = e + 1
        sa, sb = lower(d)
        sel = (mask[sa] >> e & 1).astype(bool)
        if not sel.any():
            continue
        fa, fb = f[sa][sel], f[sb][sel]
        with np.errstate(all="ignore"):
            t = fa / (fa - fb)
        n_t1 += int((t == 1.0).sum())
        p = lin[sa][sel]
        slot = off[p] + POPCOUNT[mflat[p] & ((1 << e) - 1)]
        for A in range(3):
            iA = idx[A][sa][sel].astype(np.float64)
            X[slot, A] = lo[A] + (iA + t) * dx if d >> A & 1 else lo[A] + iA * dx

    # ---- triangles: per cell, tetrahedron and inside pattern
    cs = tuple(slice(0, shape[A] - 1) for A in range(3))  # lower corners of the cells
    cell_lin = lin[cs]
    corner = lambda o: inside[tuple(slice(o >> A & 1, shape[A] - 1 + (o >> A & 1)) for A in range(3))]
    byte = np.zeros(cell_lin.shape, dtype=np.int64)
    for o in range(8):
        byte |= corner(o).astype(np.int64) << o
    crossed_cells = int(((byte != 0) & (byte != 255)).sum())
    tri_nodes, tri_key = [], []
    for t in range(6):
        offs = tet_offsets(t)
        code = np.zeros(cell_lin.shape, dtype=np.int64)
        for m in range(4):
            code |= (byte >> offs[m] & 1) << m
        for val in range(1, 15):
            sel = code == val
            if not sel.any():
                continue
            c0 = cell_lin[sel]
            for q, tri in enumerate(tet_triangles(val, TET_NEGATIVE[t])):
                ids = []
                for u, v in tri:
                    o, e = offs[u], (offs[v] ^ offs[u]) - 1
                    base = c0 + (o & 1) + NX * ((o >> 1 & 1) + NY * (o >> 2 & 1))
                    assert np.all(mflat[base] >> e & 1)
                    ids.append(off[base] + POPCOUNT[mflat[base] & ((1 << e) - 1)] + 1)
                tri_nodes.append(np.stack(ids, axis=1))
                tri_key.append((c0 * 6 + t) * 2 + q)
    if tri_nodes:
        order = np.argsort(np.concatenate(tri_key), kind="stable")
        E = np.asfortranarray(np.concatenate(tri_nodes)[order].astype(np.int32))
    else:
        E = np.zeros((0, 3), dtype=np.int32, order="F")
    return X, E, [nn, len(E), crossed_cells, n_t1]


def census(phi, iso=0.0):
    """(crossed edges per edge type [7], occurrences per tetrahedron and inside pattern [6][16]): what a test field exercises."""
    phi = np.asarray(phi, dtype=np.float64)
    shape = phi.shape
    with np.errstate(invalid="ignore", over="ignore"):
        inside = (phi - np.float64(iso)) < 0
    types = []
    for e in range(7):
        d = e + 1
        sa = tuple(slice(0, shape[A] - (d >> A & 1)) for A in range(3))
        sb = tuple(slice(d >> A & 1, shape[A]) for A in range(3))
        types.append(int((inside[sa] != inside[sb]).sum()))
    corner = lambda o: inside[tuple(slice(o >> A & 1, shape[A] - 1 + (o >> A & 1)) for A in range(3))]
    codes = []
    for t in range(6):
        code = sum(corner(o).astype(np.int64) << m for m, o in enumerate(tet_offsets(t)))
        codes.append(np.bincount(code.ravel(), minlength=16).tolist())
    return types, codes


# ---------------------------------------------------------------------------------- what the tests ask of a mesh
def edge_use(E):
    """{(a, b): [forward traversals, backward traversals]} over the directed sides of the triangles, a < b."""
    E = np.asarray(E, dtype=np.int64)
    a = np.concatenate([E[:, 0], E[:, 1], E[:, 2]])
    b = np.concatenate([E[:, 1], E[:, 2], E[:, 0]])
    fwd = a < b
    key = np.where(fwd, a, b) * (int(E.max()) + 1 if len(E) else 1) + np.where(fwd, b, a)
    uniq, inv = np.unique(key, return_inverse=True)
    use = np.zeros((len(uniq), 2), dtype=np.int64)
    np.add.at(use, (inv.ravel(), np.where(fwd, 0, 1)), 1)
    lo_hi = np.stack([uniq // (int(E.max()) + 1 if len(E) else 1), uniq % (int(E.max()) + 1 if len(E) else 1)], axis=1)
    return lo_hi, use


def open_edges(E):
    """The node pairs of the sides that are not shared by exactly two triangles in opposite directions."""
    lo_hi, use = edge_use(E)
    return lo_hi[~((use[:, 0] == 1) & (use[:, 1] == 1))]


def components(nn, E):
    """Number of connected components of the nodes used by E (union-find over triangle sides)."""
    parent = np.arange(nn + 1)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for tri in np.asarray(E):
        r = find(int(tri[0]))
        for v in tri[1:]:
            s = find(int(v))
            if s != r:
                parent[s] = r
    return len({find(int(v)) for v in np.unique(E)})


def wavy(shape, dx, lo=-1.5):
    """A perturbation that bends a sphere field enough for all seven edge types and every tetrahedron pattern to occur."""
    x, y, z = (lo + dx * np.arange(n) for n in shape)
    return 0.11 * np.sin(5.3 * x[:, None, None] + 1.1) * np.cos(4.1 * y[None, :, None] - 0.4) * np.sin(3.7 * z[None, None, :] + 0.3)
