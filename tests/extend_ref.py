"""Serial restatement of lsf_extend_field (include/lsf.h): a quantity q carried off a frozen set constant along the normals of phi,
grad(q) . grad(phi) = 0, first-order upwind in |phi|, by rounds of 8 raster sweeps.

Three forms of the same loops, as in distance_fill_ref.py:
  extend_loops   the plain triple loop, one point at a time, in raster order -- the contract read aloud;
  extend         numpy, vectorised over the hyperplanes of the sweep's reflected frame.  A point reads its six axis neighbours only;
                 the three upstream ones lie on the hyperplane before, the three downstream ones on the one after, so visiting
                 hyperplane by hyperplane gives every point exactly the operands the raster order gives it;
  extend_tiles   the schedule of the GPU kernel run serially (tile planes, private tile copies with a halo snapshot per tile plane,
                 in-tile hyperplanes): the ordering argument of DESIGN.md section 4.14 as a program.
All evaluate the visit exactly as the contract writes it (numpy fuses nothing; / is IEEE), so they agree bit for bit, and the GPU
tests compare with `extend`.

Layout: q and phi are (nx+1, ny+1, nz+1).  Returns (field, rounds_done, changed_trace, (frozen, reached, unreached)); the inputs are
not modified.  Unknown is NaN.  Also here: the inputs the tests share.
"""
import functools

import numpy as np

import distance_fill_ref as D

DIRECTIONS = D.DIRECTIONS
frozen_set = D.frozen_set


def check(q, phi, frozen):
    """(frozen points, non-finite q on frozen points, non-finite phi anywhere): what the library counts before it writes."""
    return int(frozen.sum()), int((frozen & ~np.isfinite(q)).sum()), int((~np.isfinite(phi)).sum())


def _start(q, phi, dx, band, mask):
    q = np.asarray(q, dtype=np.float64)
    phi = np.asarray(phi, dtype=np.float64)
    frozen = frozen_set(phi, np.float64(dx), band, mask)
    F = np.full(tuple(s + 2 for s in phi.shape), np.inf)  # |phi| with a ring of +inf: a neighbour outside the grid
    F[1:-1, 1:-1, 1:-1] = np.abs(phi)
    Q = np.full(F.shape, np.nan)  # q with the non-frozen points unknown
    Q[1:-1, 1:-1, 1:-1] = np.where(frozen, q, np.nan)
    return frozen, F, Q


def _finish(frozen, Q, trace):
    out = np.ascontiguousarray(Q[1:-1, 1:-1, 1:-1])
    nan = np.isnan(out)
    return out, len(trace), trace, (int(frozen.sum()), int((~frozen & ~nan).sum()), int((~frozen & nan).sum()))


def _visit(fp, axes):
    """One visit.  axes: per axis (f, q) of the neighbour at the lower index, then of the one at the higher.  The new value, or None
    when no axis is used."""
    s, t = [], []
    for f_lo, q_lo, f_hi, q_hi in axes:
        fn, qn = (f_hi, q_hi) if f_hi < f_lo else (f_lo, q_lo)
        w = fp - fn
        if w > 0 and not np.isnan(qn):
            s.append(w)
            t.append(w * qn)
        else:
            s.append(np.float64(0.0))
            t.append(np.float64(0.0))
    den = (s[0] + s[1]) + s[2]
    if den == 0:
        return None
    return ((t[0] + t[1]) + t[2]) / den


def _axes(F, Q, I, J, K, i, j, k):
    """The operands of _visit for the point (I, J, K) of F and (i, j, k) of Q."""
    return ((F[I - 1, J, K], Q[i - 1, j, k], F[I + 1, J, K], Q[i + 1, j, k]),
            (F[I, J - 1, K], Q[i, j - 1, k], F[I, J + 1, K], Q[i, j + 1, k]),
            (F[I, J, K - 1], Q[i, j, k - 1], F[I, J, K + 1], Q[i, j, k + 1]))


def extend_loops(q, phi, dx, band=None, mask=None, max_rounds=64):
    frozen, F, Q = _start(q, phi, dx, band, mask)
    NX, NY, NZ = frozen.shape
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
                        new = _visit(F[I, J, K], _axes(F, Q, I, J, K, I, J, K))
                        if new is not None and not (new == Q[I, J, K]):
                            Q[I, J, K] = new
                            changed += 1
        trace.append(changed)
        if changed == 0:
            break
    return _finish(frozen, Q, trace)


def extend(q, phi, dx, band=None, mask=None, max_rounds=64):
    frozen, F, Q = _start(q, phi, dx, band, mask)
    NX, NY, NZ = frozen.shape
    strides = ((NY + 2) * (NZ + 2), NZ + 2, 1)  # of the C-ordered padded arrays
    live = ~frozen
    i, j, k = (v[live] for v in np.meshgrid(np.arange(NX), np.arange(NY), np.arange(NZ), indexing="ij"))
    flat = np.ravel_multi_index((i + 1, j + 1, k + 1), F.shape)
    f = F.reshape(-1)
    # |phi| never changes: the neighbour each axis takes and its weight are fixed for the whole call
    nb, w = [], []
    with np.errstate(invalid="ignore"):
        for st in strides:
            hi = f[flat + st] < f[flat - st]  # a tie takes the lower index
            n = np.where(hi, flat + st, flat - st)
            nb.append(n)
            w.append(f[flat] - f[n])
    plans = {}
    for d in DIRECTIONS:
        s = sum((c if sg > 0 else (m - 1 - c)) for c, sg, m in zip((i, j, k), d, (NX, NY, NZ)))
        order = np.argsort(s, kind="stable")
        cuts = np.searchsorted(s[order], np.arange(NX + NY + NZ - 1))
        plans[d] = [order[cuts[p]:cuts[p + 1]] for p in range(NX + NY + NZ - 2)]
    v = Q.reshape(-1)
    trace = []
    with np.errstate(invalid="ignore", divide="ignore"):
        while len(trace) < max_rounds:
            changed = 0
            for d in DIRECTIONS:
                for sel in plans[d]:
                    if sel.size == 0:
                        continue
                    s, t = [], []
                    for a in range(3):
                        qn, wa = v[nb[a][sel]], w[a][sel]
                        used = (wa > 0) & ~np.isnan(qn)
                        s.append(np.where(used, wa, 0.0))
                        t.append(np.where(used, wa * qn, 0.0))
                    den = (s[0] + s[1]) + s[2]
                    new = ((t[0] + t[1]) + t[2]) / den
                    idx = flat[sel]
                    store = (den != 0) & ~(new == v[idx])
                    v[idx[store]] = new[store]
                    changed += int(store.sum())
            trace.append(changed)
            if changed == 0:
                break
    return _finish(frozen, Q, trace)


def extend_tiles(q, phi, dx, band=None, mask=None, max_rounds=64, tile=(32, 8, 8)):
    """The schedule of the GPU kernel, serially: tiles in hyperplane order A + B + C of the reflected frame; a tile works on a
    private copy of q on its points and its six face halos taken when its turn comes, visits its cells by in-tile hyperplanes
    a + b + c (all reads of a step before its writes), and copies its cells back.  Tiles of one plane are taken one after the
    other here; that they could run side by side is the claim under test: none reads what another one of its plane writes.
    (|phi| is never written, so it is read in place.)"""
    frozen, F, Q = _start(q, phi, dx, band, mask)
    n = frozen.shape
    nT = [-(-n[a] // tile[a]) for a in range(3)]
    trace = []
    while len(trace) < max_rounds:
        changed = 0
        for d in DIRECTIONS:
            for P in range(sum(nT) - 2):
                snapshot = Q.copy()  # what the tiles of this plane may read from outside themselves
                for B in range(nT[1]):
                    for C in range(nT[2]):
                        A = P - B - C
                        if A < 0 or A >= nT[0]:
                            continue
                        t = [T if s > 0 else nT[a] - 1 - T for a, (T, s) in enumerate(zip((A, B, C), d))]
                        o = [t[a] * tile[a] for a in range(3)]
                        u = np.full(tuple(v + 2 for v in tile), 12345.0)  # corners, edges and cells past the grid: never used
                        own = tuple(slice(o[a] + 1, min(o[a] + tile[a], n[a]) + 1) for a in range(3))
                        ext = tuple(v.stop - v.start for v in own)
                        u[1:ext[0] + 1, 1:ext[1] + 1, 1:ext[2] + 1] = snapshot[own]
                        for a in range(3):
                            for side, src in ((0, o[a]), (tile[a] + 1, o[a] + tile[a] + 1)):
                                sl, sg = [slice(1, ext[0] + 1), slice(1, ext[1] + 1), slice(1, ext[2] + 1)], list(own)
                                sl[a], sg[a] = side, min(src, n[a] + 1)
                                u[tuple(sl)] = snapshot[tuple(sg)]
                        for a in range(3):  # the face of a partial tile that lies past the grid: the ring (w = -inf: never used)
                            if ext[a] < tile[a]:
                                sl = [slice(1, ext[0] + 1), slice(1, ext[1] + 1), slice(1, ext[2] + 1)]
                                sl[a] = ext[a] + 1
                                u[tuple(sl)] = np.nan
                        for p in range(sum(tile) - 2):
                            writes = []
                            for b in range(tile[1]):
                                for c in range(tile[2]):
                                    a_ = p - b - c
                                    if a_ < 0 or a_ >= tile[0]:
                                        continue
                                    l = [m if s > 0 else tile[x] - 1 - m for x, (m, s) in enumerate(zip((a_, b, c), d))]
                                    if any(l[x] >= ext[x] for x in range(3)) or frozen[o[0] + l[0], o[1] + l[1], o[2] + l[2]]:
                                        continue
                                    i, j, k = l[0] + 1, l[1] + 1, l[2] + 1
                                    I, J, K = o[0] + i, o[1] + j, o[2] + k
                                    axes = _axes(F, u, I, J, K, i, j, k)
                                    assert not any(x[1] == 12345.0 or x[3] == 12345.0 for x in axes)
                                    new = _visit(F[I, J, K], axes)
                                    if new is not None and not (new == u[i, j, k]):
                                        writes.append((i, j, k, new))
                            for i, j, k, new in writes:
                                u[i, j, k] = new
                            changed += len(writes)
                        Q[own] = u[1:ext[0] + 1, 1:ext[1] + 1, 1:ext[2] + 1]
        trace.append(changed)
        if changed == 0:
            break
    return _finish(frozen, Q, trace)


# ------------------------------------------------------------------------------------------------ the inputs the tests share
CASES = ("tiny", "thin", "long", "sphere15", "twospheres")  # names of distance_fill_ref.CASES


def quantity(shape, dx):
    """1 + 0.5 x - 0.3 y + 0.2 z^2 at the grid coordinates (i, j, k) * dx."""
    x, y, z = (np.arange(m) * np.float64(dx) for m in shape)
    X, Y, Z = np.meshgrid(x, y, z, indexing="ij")
    return 1.0 + 0.5 * X - 0.3 * Y + 0.2 * Z * Z


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(q, phi, dx, band) of a named case, all read-only: phi is the exact distance of distance_fill_ref's input, q the quantity
    above on the frozen points -- with a 0.0, a -0.0 and a negative value planted on three of them -- and 7.0 on every other
    point, one of which holds NaN: what a non-frozen point holds on entry is ignored."""
    name, band = D.CASES[case]
    phi, dx = D.exact(name)
    frozen = frozen_set(phi, dx, band=band)
    q = np.where(frozen, quantity(phi.shape, dx), 7.0)
    at = np.argwhere(frozen)
    assert len(at) >= 3
    for m, v in zip((0, len(at) // 2, len(at) - 1), (0.0, -0.0, -2.5)):
        q[tuple(at[m])] = v
    q[tuple(np.argwhere(~frozen)[len(np.argwhere(~frozen)) // 3])] = np.nan
    q.setflags(write=False)
    phi.setflags(write=False)
    return q, phi, dx, band


@functools.lru_cache(maxsize=None)
def want(case, cap):
    q, phi, dx, band = inputs(case)
    out = extend(q, phi, dx, band=band, max_rounds=cap)
    out[0].setflags(write=False)
    return out


def sphere_case(N, clamp_cells=None):
    """(q, phi, dx, r, X, Y, Z) of the closed-form case: a sphere of radius 0.7 about the origin on N points per axis of
    [-1.5, 1.5], shifted by (0.013, -0.02, 0.031); q = 1 + 0.5 X/r - 0.3 Y/r + 0.2 (Z/r)^2 is constant along the normals."""
    dx = np.float64(3.0) / (N - 1)
    ax = [-1.5 + s + np.arange(N) * dx for s in (0.013, -0.02, 0.031)]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    r = np.sqrt(X * X + Y * Y + Z * Z)
    phi = r - 0.7
    if clamp_cells is not None:
        phi = D.clamp(phi, dx, clamp_cells)
    q = 1.0 + 0.5 * X / r - 0.3 * Y / r + 0.2 * (Z / r) ** 2
    return q, phi, dx
