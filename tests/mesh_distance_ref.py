"""numpy reference for lsf_mesh_distance (include/lsf.h): the signed distance of every grid point to every triangle, all pairs.

Written independently of the library's scatter: no boxes, no keys, no region tests by products of dot products.  Per
triangle the closest point is the foot of the perpendicular when it falls inside the triangle (2 x 2 solve for its
barycentric coordinates), otherwise the nearest of the three clamped projections onto its sides; a clamp at an end names
the vertex as the closest feature.  The sign is that of the dot product of the offset with the angle-weighted pseudonormal
of that feature (Baerentzen & Aanaes 2005), zero counting as positive.  Between triangles the smaller distance wins and,
at equal distance, the positive sign.  Also here: the closed-form distance of an axis-aligned box, the clamp + column fill
of the contract in numpy, and the icosphere of the tests.
"""
import numpy as np


def grid_points(n, dx, xLo):
    """(nx+1, ny+1, nz+1, 3) coordinates xLo + i*dx (set3d.f90:168-170); n = (nx, ny, nz)."""
    ax = [np.float64(xLo[a]) + np.arange(n[a] + 1) * np.float64(dx) for a in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1)


def box_distance(P, lo, hi):
    """Closed-form signed distance to the axis-aligned box [lo, hi], negative inside."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    q = np.maximum(lo - P, P - hi)  # per axis: > 0 outside the slab
    outside = np.sqrt((np.maximum(q, 0.0) ** 2).sum(axis=-1))
    return np.where((q <= 0).all(axis=-1), q.max(axis=-1), outside)


def _unit(v):
    return v / np.linalg.norm(v)


def pseudonormals(X, E):
    """Unit face normals, edge pseudonormals (ntri,3: sides 01, 12, 20), vertex pseudonormals (nnode,3) and the mask of
    non-degenerate triangles.  X (nnode,3) float64, E (ntri,3) 1-based."""
    T = X[np.asarray(E) - 1]
    nrm = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    ln = np.linalg.norm(nrm, axis=1)
    ok = ln > 0
    fn = np.zeros_like(nrm)
    fn[ok] = nrm[ok] / ln[ok, None]
    vn = np.zeros_like(X)
    sides = {}
    for t in np.flatnonzero(ok):
        ids = [int(v) - 1 for v in E[t]]
        for c in range(3):
            u, w = T[t, (c + 1) % 3] - T[t, c], T[t, (c + 2) % 3] - T[t, c]
            vn[ids[c]] += np.arctan2(np.linalg.norm(np.cross(u, w)), u @ w) * fn[t]
            sides.setdefault((min(ids[c], ids[(c + 1) % 3]), max(ids[c], ids[(c + 1) % 3])), []).append(t)
    en = np.zeros((len(E), 3, 3))
    for t in np.flatnonzero(ok):
        ids = [int(v) - 1 for v in E[t]]
        for c in range(3):
            ts = sides[(min(ids[c], ids[(c + 1) % 3]), max(ids[c], ids[(c + 1) % 3]))]
            en[t, c] = fn[ts[0]] + fn[ts[1]] if len(ts) == 2 else fn[t]
    return fn, en, vn, ok


def signed_distance(P, X, E, signed=True, within=None):
    """Signed (or unsigned) distance of the points P (..., 3) to the mesh, all pairs.  within: leave out the triangles whose
    bounding box is farther than this from the bounding box of P (values up to `within` are unaffected, larger ones stay
    larger: enough for a clamped comparison, and what keeps a mesh of many triangles affordable)."""
    X = np.asarray(X, dtype=np.float64)
    E = np.asarray(E)
    shape = P.shape[:-1]
    Q = P.reshape(-1, 3)
    fn, en, vn, ok = pseudonormals(X, E)
    best_d = np.full(Q.shape[0], np.inf)
    best_neg = np.zeros(Q.shape[0], dtype=bool)
    if within is not None:
        T = X[E - 1]
        gap = np.maximum(np.maximum(Q.min(axis=0) - T.max(axis=1), T.min(axis=1) - Q.max(axis=0)), 0.0)
        ok = ok & (np.sqrt((gap * gap).sum(axis=1)) <= within)
    for t in np.flatnonzero(ok):
        ids = [int(v) - 1 for v in E[t]]
        V = X[ids]
        # foot of the perpendicular in the triangle's own frame
        e0, e1 = V[1] - V[0], V[2] - V[0]
        G = np.array([[e0 @ e0, e0 @ e1], [e0 @ e1, e1 @ e1]])
        r = Q - V[0]
        uv = np.linalg.solve(G, np.stack([r @ e0, r @ e1]))
        inside = (uv[0] >= 0) & (uv[1] >= 0) & (uv[0] + uv[1] <= 1)
        hgt = r @ fn[t]
        d = np.where(inside, np.abs(hgt), np.inf)
        s = np.where(inside, hgt, 0.0)
        for c in range(3):
            a, b = V[c], V[(c + 1) % 3]
            ab = b - a
            tt = np.clip(((Q - a) @ ab) / (ab @ ab), 0.0, 1.0)
            off = Q - (a + tt[:, None] * ab)
            dc = np.sqrt((off * off).sum(axis=1))
            pn = np.where((tt == 0.0)[:, None], vn[ids[c]], np.where((tt == 1.0)[:, None], vn[ids[(c + 1) % 3]], en[t, c]))
            sc = (off * pn).sum(axis=1)
            take = ~inside & (dc < d)
            d = np.where(take, dc, d)
            s = np.where(take, sc, s)
        neg = (s < 0) if signed else np.zeros_like(inside)
        better = (d < best_d) | ((d == best_d) & best_neg & ~neg)
        best_d = np.where(better, d, best_d)
        best_neg = np.where(better, neg, best_neg)
    return np.where(best_neg, -best_d, best_d).reshape(shape)


def signed_volume(X, E):
    T = np.asarray(X, dtype=np.float64)[np.asarray(E) - 1]
    return float((T[:, 0] * np.cross(T[:, 1], T[:, 2])).sum() / 6.0)


def clamp_columns(sd, far, exterior=1.0):
    """The contract's field from an exact signed distance sd (nx+1, ny+1, nz+1): sd where |sd| <= far, +-far elsewhere with
    the sign of the last tube point below in the (i,j) column, `exterior` in front of the first.  Returns (field, tube)."""
    tube = np.abs(sd) <= far
    k = np.arange(sd.shape[2])
    last = np.maximum.accumulate(np.where(tube, k, -1), axis=2)  # index of the last tube point at or below k
    sgn_at = np.where(np.signbit(sd), -1.0, 1.0)
    carried = np.take_along_axis(sgn_at, np.maximum(last, 0), axis=2)
    carried = np.where(last < 0, exterior, carried)
    return np.where(tube, sd, carried * far), tube


def icosphere(subdiv=2, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """Subdivided icosahedron, outward winding: (X (nnode,3) float64, E (ntri,3) int32 1-based); 20 * 4^subdiv triangles."""
    t = (1.0 + np.sqrt(5.0)) / 2.0
    V = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    V = [_unit(np.array(v, dtype=np.float64)) for v in V]
    Fc = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
          (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdiv):
        mid, out = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                V.append(_unit(V[a] + V[b]))
                mid[key] = len(V) - 1
            return mid[key]

        for a, b, c in Fc:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        Fc = out
    X = np.array(V) * radius + np.asarray(centre, dtype=np.float64)
    return X, np.array(Fc, dtype=np.int32) + 1
