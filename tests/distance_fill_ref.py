"""Serial restatement of lsf_distance_fill (include/lsf.h): first-order Godunov fast sweeping outwards from a frozen set.

Three forms of the same loops:
  fill_loops   the plain triple loop, one point at a time, in raster order -- the contract read aloud;
  fill         numpy, vectorised over the hyperplanes i + j + k of the sweep's reflected frame.  A point reads its six axis
               neighbours only; the three upstream ones lie on the hyperplane before, the three downstream ones on the one after, so
               visiting hyperplane by hyperplane gives every point exactly the operands the raster order gives it.
  fill_tiles   the schedule of the GPU kernel run serially (tile planes, private tile copies, in-tile hyperplanes): the ordering
               argument of DESIGN.md section 4.11 as a program.
All evaluate the update exactly as the contract writes it (numpy fuses nothing; sqrt and / are IEEE), so they agree bit for bit,
and the GPU tests compare with `fill`.

Layout: phi is (nx+1, ny+1, nz+1).  Returns (field, rounds_done, changed_trace, frozen_points); the input is not modified.
Also here: the inputs the tests share.
"""
import numpy as np

# the reference's direction order (subs.f90:740-855)
DIRECTIONS = ((+1, +1, +1), (+1, +1, -1), (+1, -1, -1), (-1, -1, -1), (-1, +1, -1), (-1, -1, +1), (-1, +1, +1), (+1, -1, +1))


def frozen_set(phi, dx, band=None, mask=None):
    assert (band is None) != (mask is None)
    if mask is not None:
        return np.asarray(mask) == 1
    far = np.float64(band) * np.float64(dx)
    return np.abs(phi) < far


def check(phi, frozen):
    """(frozen points, non-finite frozen values, pairs of axis neighbours of opposite sign that are not both frozen)."""
    neg = phi < 0
    jumps = 0
    for ax in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        jumps += int(((neg[lo] != neg[hi]) & ~(frozen[lo] & frozen[hi])).sum())
    return int(frozen.sum()), int((frozen & ~np.isfinite(phi)).sum()), jumps


def _solve_scalar(x, y, z, dx):
    a = min(min(x, y), z)
    c = max(max(x, y), z)
    b = max(min(x, y), min(max(x, y), z))
    t = a + dx
    if t > b:
        d = a - b
        t = ((a + b) + np.sqrt(2 * (dx * dx) - d * d)) * 0.5
        if t > c:
            t = (((a + b) + c) + np.sqrt(max(3 * (dx * dx) - (((a - b) * (a - b) + (a - c) * (a - c)) + (b - c) * (b - c)), 0))) / 3
    return t


def _start(phi, dx, band, mask):
    phi = np.asarray(phi, dtype=np.float64)
    dx = np.float64(dx)
    frozen = frozen_set(phi, dx, band, mask)
    neg = phi < 0
    U = np.full(tuple(s + 2 for s in phi.shape), np.inf)  # magnitudes with a ring of +inf: a neighbour outside the grid
    U[1:-1, 1:-1, 1:-1] = np.where(frozen, np.abs(phi), np.inf)
    return phi, dx, frozen, neg, U


def _finish(phi, frozen, neg, U, rounds, trace):
    u = U[1:-1, 1:-1, 1:-1]
    return np.where(frozen, phi, np.where(neg, -u, u)), rounds, trace, int(frozen.sum())


def fill_loops(phi, dx, band=None, mask=None, max_rounds=64):
    phi, dx, frozen, neg, U = _start(phi, dx, band, mask)
    NX, NY, NZ = phi.shape
    trace = []
    while len(trace) < max_rounds:
        changed = 0
        for sx, sy, sz in DIRECTIONS:
            for k in (range(NZ) if sz > 0 else range(NZ - 1, -1, -1)):
                for j in (range(NY) if sy > 0 else range(NY - 1, -1, -1)):
                    for i in (range(NX) if sx > 0 else range(NX - 1, -1, -1)):
                        if frozen[i, j, k]:
                            continue
                        I, J, K = i + 1, j + 1, k + 1
                        x = min(U[I - 1, J, K], U[I + 1, J, K])
                        y = min(U[I, J - 1, K], U[I, J + 1, K])
                        z = min(U[I, J, K - 1], U[I, J, K + 1])
                        if min(min(x, y), z) == np.inf:
                            continue
                        t = _solve_scalar(x, y, z, dx)
                        if t < U[I, J, K]:
                            U[I, J, K] = t
                            changed += 1
        trace.append(changed)
        if changed == 0:
            break
    return _finish(phi, frozen, neg, U, len(trace), trace)


def _planes(shape, live):
    """Flat indices (into the padded array of the reflected frame) of the live points of every hyperplane a + b + c."""
    NX, NY, NZ = shape
    a, b, c = np.meshgrid(np.arange(NX), np.arange(NY), np.arange(NZ), indexing="ij")
    s = (a + b + c)[live]
    flat = np.ravel_multi_index((a[live] + 1, b[live] + 1, c[live] + 1), (NX + 2, NY + 2, NZ + 2))
    order = np.argsort(s, kind="stable")
    s, flat = s[order], flat[order]
    cuts = np.searchsorted(s, np.arange(NX + NY + NZ - 1))
    return [flat[cuts[p]:cuts[p + 1]] for p in range(NX + NY + NZ - 2)]


def fill(phi, dx, band=None, mask=None, max_rounds=64):
    phi, dx, frozen, neg, U = _start(phi, dx, band, mask)
    shape = phi.shape
    sy_, sz_ = (shape[2] + 2), 1  # strides of the C-ordered padded array
    sx_ = (shape[1] + 2) * sy_
    plans = {}
    for d in DIRECTIONS:
        flip = tuple(slice(None, None, s) for s in d)
        plans[d] = _planes(shape, ~frozen[flip])
    dx2 = dx * dx
    trace = []
    with np.errstate(invalid="ignore"):
        while len(trace) < max_rounds:
            changed = 0
            for d in DIRECTIONS:
                V = np.ascontiguousarray(U[tuple(slice(None, None, s) for s in d)])  # the reflected frame, ring included
                v = V.reshape(-1)
                for idx in plans[d]:
                    if idx.size == 0:
                        continue
                    x = np.minimum(v[idx - sx_], v[idx + sx_])
                    y = np.minimum(v[idx - sy_], v[idx + sy_])
                    z = np.minimum(v[idx - sz_], v[idx + sz_])
                    a = np.minimum(np.minimum(x, y), z)
                    c = np.maximum(np.maximum(x, y), z)
                    b = np.maximum(np.minimum(x, y), np.minimum(np.maximum(x, y), z))
                    ok = a < np.inf
                    t = a + dx
                    two = ok & (t > b)
                    dd = a - b
                    t2 = ((a + b) + np.sqrt(2 * dx2 - dd * dd)) * 0.5
                    t = np.where(two, t2, t)
                    three = two & (t > c)
                    s3 = ((a - b) * (a - b) + (a - c) * (a - c)) + (b - c) * (b - c)
                    t3 = (((a + b) + c) + np.sqrt(np.maximum(3 * dx2 - s3, 0))) / 3
                    t = np.where(three, t3, t)
                    old = v[idx]
                    low = ok & (t < old)
                    v[idx[low]] = t[low]
                    changed += int(low.sum())
                U = V[tuple(slice(None, None, s) for s in d)]
            trace.append(changed)
            if changed == 0:
                break
    return _finish(phi, frozen, neg, np.ascontiguousarray(U), len(trace), trace)


def fill_tiles(phi, dx, band=None, mask=None, max_rounds=64, tile=(32, 8, 8)):
    """The schedule of the GPU kernel, serially: tiles in hyperplane order A + B + C of the reflected frame; a tile works on a
    private copy of its points and its six face halos taken when its turn comes, visits its cells by in-tile hyperplanes
    a + b + c (all reads of a step before its writes), and copies its cells back.  Tiles of one plane are taken one after the
    other here; that they could run side by side is the claim under test: none reads what another one of its plane writes."""
    phi, dx, frozen, neg, U = _start(phi, dx, band, mask)
    n = phi.shape
    nT = [-(-n[a] // tile[a]) for a in range(3)]
    trace = []
    while len(trace) < max_rounds:
        changed = 0
        for d in DIRECTIONS:
            for P in range(sum(nT) - 2):
                snapshot = U.copy()  # what the tiles of this plane may read from outside themselves
                for B in range(nT[1]):
                    for C in range(nT[2]):
                        A = P - B - C
                        if A < 0 or A >= nT[0]:
                            continue
                        t = [T if s > 0 else nT[a] - 1 - T for a, (T, s) in enumerate(zip((A, B, C), d))]
                        o = [t[a] * tile[a] for a in range(3)]
                        u = np.full(tuple(v + 2 for v in tile), np.nan)  # corners and edges stay NaN: a star never reads them
                        own = tuple(slice(o[a] + 1, min(o[a] + tile[a], n[a]) + 1) for a in range(3))
                        ext = tuple(v.stop - v.start for v in own)
                        u[1:ext[0] + 1, 1:ext[1] + 1, 1:ext[2] + 1] = snapshot[own]
                        for a in range(3):
                            for side, src in ((0, o[a]), (tile[a] + 1, o[a] + tile[a] + 1)):
                                sl, sg = [slice(1, ext[0] + 1), slice(1, ext[1] + 1), slice(1, ext[2] + 1)], list(own)
                                sl[a], sg[a] = side, min(src, n[a] + 1)
                                u[tuple(sl)] = snapshot[tuple(sg)]
                        # cells past the grid inside a partial tile: +inf like the ring
                        u[ext[0] + 1:tile[0] + 1, 1:-1, 1:-1] = np.inf
                        u[1:-1, ext[1] + 1:tile[1] + 1, 1:-1] = np.inf
                        u[1:-1, 1:-1, ext[2] + 1:tile[2] + 1] = np.inf
                        for p in range(sum(tile) - 2):
                            writes = []
                            for b in range(tile[1]):
                                for c in range(tile[2]):
                                    a_ = p - b - c
                                    if a_ < 0 or a_ >= tile[0]:
                                        continue
                                    l = [q if s > 0 else tile[m] - 1 - q for m, (q, s) in enumerate(zip((a_, b, c), d))]
                                    if any(l[m] >= ext[m] for m in range(3)) or frozen[o[0] + l[0], o[1] + l[1], o[2] + l[2]]:
                                        continue
                                    I, J, K = l[0] + 1, l[1] + 1, l[2] + 1
                                    x = min(u[I - 1, J, K], u[I + 1, J, K])
                                    y = min(u[I, J - 1, K], u[I, J + 1, K])
                                    z = min(u[I, J, K - 1], u[I, J, K + 1])
                                    assert not (np.isnan(x) or np.isnan(y) or np.isnan(z))
                                    if min(min(x, y), z) == np.inf:
                                        continue
                                    v = _solve_scalar(x, y, z, dx)
                                    if v < u[I, J, K]:
                                        writes.append((I, J, K, v))
                            for I, J, K, v in writes:
                                u[I, J, K] = v
                            changed += len(writes)
                        U[own] = u[1:ext[0] + 1, 1:ext[1] + 1, 1:ext[2] + 1]
        trace.append(changed)
        if changed == 0:
            break
    return _finish(phi, frozen, neg, U, len(trace), trace)


# ------------------------------------------------------------------------------------------------ the inputs the tests share
def grid_points(npts, dx, xLo):
    """(NX, NY, NZ, 3) coordinates xLo + i*dx of a grid of npts points."""
    ax = [np.float64(xLo[a]) + np.arange(npts[a]) * np.float64(dx) for a in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1)


def box_distance(P, lo, hi):
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    q = np.maximum(lo - P, P - hi)
    return np.where((q <= 0).all(axis=-1), q.max(axis=-1), np.sqrt((np.maximum(q, 0.0) ** 2).sum(axis=-1)))


def sphere_distance(P, centre, radius):
    return np.linalg.norm(P - np.asarray(centre, dtype=np.float64), axis=-1) - radius


def clamp(ref, dx, width):
    """The exact distance inside |ref| < width*dx, +-width*dx elsewhere: what lsf_mesh_distance leaves."""
    far = np.float64(width) * np.float64(dx)
    return np.where(np.abs(ref) < far, ref, np.where(ref < 0, -far, far))


def exact(name):
    """(exact signed distance, dx) of the named input."""
    if name == "box":  # cube40's box on its 62^3 grid
        dx, npts, xLo = 0.05, (62, 62, 62), (-1.5, -1.5, -1.5)
        return box_distance(grid_points(npts, dx, xLo), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), dx
    if name == "sphere":
        dx, npts, xLo = 0.07, (41, 34, 28), (-1.02, -0.5, -0.93)
        return sphere_distance(grid_points(npts, dx, xLo), (0.33, -0.27, 0.071), 0.61), dx
    dx, xLo = 0.07, (-1.02, -0.5, -0.93)

    def two(npts):  # the second sphere leaves the grid through walls
        P = grid_points(npts, dx, xLo)
        return np.minimum(sphere_distance(P, (-0.3, 0.4, 0.2), 0.35), sphere_distance(P, (1.0, 1.0, 0.3), 0.4))

    if name == "twospheres":
        return two((41, 34, 28)), dx
    if name == "thin":  # an axis thinner than a tile
        return two((41, 34, 28))[:, :, 12:17].copy(), dx
    if name == "tiny":
        return sphere_distance(grid_points((8, 7, 3), 0.2, (-0.7, -0.6, -0.2)), (0.05, 0.02, 0.1), 0.45), 0.2
    if name == "long":  # three tiles in x, partial last tiles
        return sphere_distance(grid_points((70, 19, 21), 0.05, (-1.7, -0.45, -0.5)), (0.11, 0.03, -0.02), 0.3), 0.05
    raise KeyError(name)


# name -> (input of exact(), width in cells)
CASES = {"box35": ("box", 3.5), "box15": ("box", 1.5), "sphere35": ("sphere", 3.5), "sphere15": ("sphere", 1.5),
         "twospheres": ("twospheres", 2.5), "thin": ("thin", 2.5), "tiny": ("tiny", 1.5), "long": ("long", 2.5)}
