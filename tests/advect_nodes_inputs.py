"""Input sets of the node-advection and narrowBand parity tests, shared by the CPU tests (oracle, numpy statement, defects), the GPU
tests and tests/golden/make_golden_post.py.  Grids are given as POINT counts (nx+1, ny+1, nz+1); every set is deterministic.

Node sets of `case(name)` (phi, phiSB, nodes, iters):
  synth-post-K          the fixture synth_post_37x29x23.npz (the reference's own run), K = 0, 1, 2, 1000 passes
  cells-GRID-MASK       one node per admissible cell, one pass; MASK = ones | zeros (3 passes) | bernoulli (with entries 7 and -1)
  cells-13x11x9-negated the same nodes on -phi: phiSurf < 0, nothing moves
  cells-13x11x9-nan     one NaN in phi
  special-13x11x9       nodes exactly on grid points, at offsets of exactly 0.5, and at x = -0.0 (also run on -phi: special-...-negated)
  threshold-13x11x9     nodes on grid points whose phi is 1e-13 and its two neighbours in double
  sphere-131x127x140    2 329 180 points: the gradient kernel's grid-stride loop makes a second trip
"""
from __future__ import annotations

import collections
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POST_FIXTURE = os.path.join(GOLDEN, "synth_post_37x29x23.npz")

Case = collections.namedtuple("Case", "phi sb n dx xLo nodes iters")  # n = (nx, ny, nz); phi, sb, nodes Fortran-ordered

# ------------------------------------------------------------------------------------------------ the fixture's input
POST_NPTS, POST_DX, POST_XLO = (37, 29, 23), 0.08, (-1.3, -1.1, -0.9)
# Moved from the issue's (0.1, 0.0, -0.05) / 0.45: 23 points in z cannot hold a band of +-8.1 dx around ANY closed surface with 4
# planes to spare, so the generator pads phi with zero planes instead (see its docstring) and this smaller sphere keeps every
# gradient that a NODE interpolates clear of that padding: the fixture's nodes are the reference's answer with no undefined read.
POST_CENTRE, POST_RADIUS, POST_NODES, POST_SEED = (0.1, -0.1, -0.02), 0.25, 1000, 20241
POST_PASSES = (0, 1, 2, 1000)


def grid_xyz(npts, dx, xLo):
    return np.meshgrid(*(xLo[a] + dx * np.arange(npts[a]) for a in range(3)), indexing="ij", sparse=True)


def sphere_nodes(count, centre, radius, dx, spread, seed, zmin=-1.0):
    """`count` seeded nodes within +-spread*dx of the sphere; the z component of the direction is uniform in [zmin, 1]"""
    rng = np.random.default_rng(seed)
    u = rng.uniform(zmin, 1.0, count)
    a = rng.uniform(0.0, 2.0 * np.pi, count)
    r = radius + rng.uniform(-spread, spread, count) * dx
    s = np.sqrt(1.0 - u * u)
    return np.asfortranarray(np.stack([centre[0] + r * s * np.cos(a), centre[1] + r * s * np.sin(a), centre[2] + r * u], axis=1))


def post_input():
    """(phi, nodes) of the fixture: distance to a sphere plus a ripple, and nodes within +-2.5 dx of the sphere"""
    x, y, z = grid_xyz(POST_NPTS, POST_DX, POST_XLO)
    c = POST_CENTRE
    phi = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - POST_RADIUS + 0.01 * np.sin(7 * x) * np.cos(5 * y)
    return np.asfortranarray(phi), sphere_nodes(POST_NODES, c, POST_RADIUS, POST_DX, 2.5, POST_SEED)


@functools.lru_cache(maxsize=None)
def post_fixture():
    return dict(np.load(POST_FIXTURE, allow_pickle=False))


# ------------------------------------------------------------------------------------------------ one node per cell
CELL_GRIDS = [(13, 11, 9), (70, 9, 12), (6, 5, 7), (3, 3, 3)]
CELL_MASKS = ["ones", "zeros", "bernoulli"]
CELL_DX, CELL_XLO = 0.08, (-0.37, 0.21, -1.03)
MOVE_BOUND = 0.7 * CELL_DX  # max|phi| = 0.3 dx * 2.2 = 0.66 dx; interpolation is a convex combination, the direction has length <= 1


def cell_phi(npts):
    """0.3 dx (1.2 + sin 7x cos 5y sin(6z + 0.3)): positive, max|phi| < 0.7 dx"""
    x, y, z = grid_xyz(npts, CELL_DX, CELL_XLO)
    return np.asfortranarray(0.3 * CELL_DX * (1.2 + np.sin(7 * x) * np.cos(5 * y) * np.sin(6 * z + 0.3)))


def cell_nodes(npts):
    """One node in each cell (i, j, k), 0 <= index <= points - 3 per axis: the cells lsf_advect_nodes admits (include/lsf.h).  Offsets
    inside the cell are uniform in [0, 1), and in [0.7, 0.95) where the index is 0, so a move shorter than 0.7 dx ends in a cell whose
    eight corners exist."""
    rng = np.random.default_rng(1000 * npts[0] + 10 * npts[1] + npts[2])
    idx = np.stack(np.meshgrid(*(np.arange(n - 2) for n in npts), indexing="ij"), axis=-1).reshape(-1, 3)
    off = np.where(idx == 0, rng.uniform(0.7, 0.95, idx.shape), rng.random(idx.shape))
    X = np.asfortranarray(np.array(CELL_XLO) + CELL_DX * (idx + off))
    assert (cell_of(X, CELL_DX, CELL_XLO) == idx).all()
    return X


def cell_of(X, dx, xLo):
    """setPhiSurf's cell index of every node (subs.f90:1082-1084)"""
    return np.floor((X - np.array(xLo)) / dx).astype(np.int64)


def admissible(X, n, dx, xLo):
    """the range lsf_advect_nodes accepts: xLo <= x < xLo + dx*(n-1) per axis, n = nx, ny, nz"""
    lo = np.array(xLo)
    return bool(((X >= lo) & (X < lo + dx * (np.array(n) - 1))).all())


def cell_mask(npts, kind):
    if kind == "ones":
        return np.ones(npts, dtype=np.int32, order="F")  # walls included: every +-4 read that wraps or leaves the allocation happens
    if kind == "zeros":
        return np.zeros(npts, dtype=np.int32, order="F")
    rng = np.random.default_rng(77 + sum(npts))
    m = (rng.random(npts) < 0.6).astype(np.int32)
    m[rng.random(npts) < 0.1] = 7   # neither 7 nor -1 is band: the reference tests `== 1`
    m[rng.random(npts) < 0.1] = -1
    return np.asfortranarray(m)


def _exact_points(npts, want):
    """`want` interior grid points (i, j, k) at which x = i*dx + xLo lands in cell i with xd == 0 exactly, on every axis"""
    ok = []
    for a in range(3):
        i = np.arange(1, npts[a] - 2)
        x = i * CELL_DX + CELL_XLO[a]
        ok.append(i[np.floor((x - CELL_XLO[a]) / CELL_DX) == i])
    pts = [(int(ok[0][q % len(ok[0])]), int(ok[1][(2 * q + 1) % len(ok[1])]), int(ok[2][(3 * q + 2) % len(ok[2])])) for q in range(want)]
    assert len(set(pts)) == want
    return np.array(pts)


def _on_points(pts):
    return np.asfortranarray(pts * CELL_DX + np.array(CELL_XLO))


THRESHOLDS = (1E-13, float(np.nextafter(1E-13, 0.0)), float(np.nextafter(1E-13, 1.0)))  # not moved, not moved, moved


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith("synth-post-"):
        g = post_fixture()
        return Case(np.asfortranarray(g["phi"]), np.asfortranarray(g["SB"].astype(np.int32)), tuple(v - 1 for v in POST_NPTS), POST_DX,
                    POST_XLO, np.asfortranarray(g["nodes_in"]), int(name.rsplit("-", 1)[1]))
    kind, grid, *rest = name.split("-")
    npts = tuple(int(v) for v in grid.split("x"))
    n = tuple(v - 1 for v in npts)
    if kind == "sphere":
        return _big(npts)
    phi, ones = cell_phi(npts), cell_mask(npts, "ones")
    if kind == "cells":
        what, nodes = rest[0], cell_nodes(npts)
        if what in CELL_MASKS:
            return Case(phi, cell_mask(npts, what), n, CELL_DX, CELL_XLO, nodes, 3 if what == "zeros" else 1)
        if what == "negated":
            return Case(-phi, ones, n, CELL_DX, CELL_XLO, nodes, 3)
        if what == "nan":
            # One NaN in phi.  The mask is 0 at the points whose stencil reads it (linear addressing): their gradient would be NaN,
            # a node interpolating it would move to NaN and the next floor() of a NaN is undefined in the reference.  With it the
            # gradient is finite everywhere; a node whose cell has the NaN point as a corner gets phiSurf = NaN and must not move.
            sx, sxy = npts[0], npts[0] * npts[1]
            at = (6, 5, 4)
            p = at[0] + sx * at[1] + sxy * at[2]
            phi, flat = phi.copy(order="F"), ones.ravel(order="F").copy()
            phi[at] = np.nan
            for s in (1, sx, sxy):
                for m in range(1, 5):
                    flat[[p - m * s, p + m * s]] = 0
            return Case(phi, np.asfortranarray(flat.reshape(npts, order="F")), n, CELL_DX, CELL_XLO, nodes, 1)
    if kind == "special":
        pts = _exact_points(npts, 6)
        half = np.asfortranarray((pts[::-1] + 0.5) * CELL_DX + np.array(CELL_XLO))
        zero = np.array([[-0.0, CELL_XLO[1] + 3.3 * CELL_DX, CELL_XLO[2] + 2.6 * CELL_DX]])
        nodes = np.asfortranarray(np.concatenate([_on_points(pts), half, zero]))
        return Case(-phi if rest else phi, ones, n, CELL_DX, CELL_XLO, nodes, 3 if rest else 1)
    if kind == "threshold":
        pts = _exact_points(npts, len(THRESHOLDS))
        phi = phi.copy(order="F")
        for q, t in zip(pts, THRESHOLDS):
            phi[tuple(q)] = t
        return Case(phi, ones, n, CELL_DX, CELL_XLO, _on_points(pts), 1)
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ second trip of the stride loop
BIG_NPTS, BIG_DX, BIG_XLO = (131, 127, 140), 0.02, (-1.3, -1.1, -0.9)
BIG_CENTRE_PT, BIG_RADIUS_PTS = (64.3, 61.6, 123.9), 7.5  # in grid points: the sphere sits under the high-z wall


def big_phi():
    x, y, z = grid_xyz(BIG_NPTS, BIG_DX, BIG_XLO)
    c = [BIG_XLO[a] + BIG_DX * BIG_CENTRE_PT[a] for a in range(3)]
    return np.asfortranarray(np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - BIG_RADIUS_PTS * BIG_DX), c


def _big(npts):
    assert npts == BIG_NPTS
    phi, c = big_phi()
    sb = np.asfortranarray((np.abs(phi) < 8.1 * BIG_DX).astype(np.int32))  # narrowBand's stencil band (the tests check it is)
    # the upper part of the sphere (direction z in [-0.2, 1]), +-1.5 dx: at least 6 dx from every wall
    nodes = sphere_nodes(500, c, BIG_RADIUS_PTS * BIG_DX, BIG_DX, 1.5, 515, zmin=-0.2)
    return Case(phi, sb, tuple(v - 1 for v in npts), BIG_DX, BIG_XLO, nodes, 1000)


def corner_max_index(c, X=None):
    """largest linear index among the eight points each node interpolates from"""
    sx, sxy = c.n[0] + 1, (c.n[0] + 1) * (c.n[1] + 1)
    ijk = cell_of(c.nodes if X is None else X, c.dx, c.xLo)
    return (ijk[:, 0] + 1) + sx * (ijk[:, 1] + 1) + sxy * (ijk[:, 2] + 1)


STRIDE_LIMIT = 8192 * 256  # points covered by one trip of the grid-stride loop of the gradient and narrowBand kernels


def expectations(name, c, got):
    """What is known about a result before anything runs (shared with the GPU tests, which pass the library's result)."""
    lo, hi = np.array(c.xLo), np.array(c.xLo) + c.dx * np.array(c.n)
    moved = (got != c.nodes).any(axis=1) | np.isnan(got).any(axis=1)
    if name.endswith(("-zeros", "-negated")):
        assert same_bits(got, c.nodes)  # the sign of a zero coordinate included
    elif name.startswith("cells-") and name.endswith("-ones"):
        # positive phi, every gradient point in the band: each node moves, by less than 0.7 dx, and stays where 8 corners exist
        assert moved.all() and np.sqrt(((got - c.nodes) ** 2).sum(axis=1)).max() < MOVE_BOUND
        assert ((got >= lo) & (got < hi)).all()
    elif name.endswith("-nan"):
        cell = cell_of(c.nodes, c.dx, c.xLo)
        at = np.argwhere(np.isnan(c.phi))[0]
        touch = ((cell <= at) & (at <= cell + 1)).all(axis=1)
        assert touch.sum() == 8 and not moved[touch].any() and moved[~touch].all() and np.isfinite(got).all()
    elif name.startswith("threshold-"):
        assert list(moved) == [False, False, True]
    elif name.startswith("special-"):
        assert moved.all()
    elif name.startswith("sphere-"):
        far = STRIDE_LIMIT
        assert c.phi.size > far and (corner_max_index(c) >= far).sum() * 3 >= len(c.nodes)
        assert (corner_max_index(c, got) >= far).sum() * 3 >= len(c.nodes) and moved.sum() * 3 >= len(c.nodes)
        assert ((c.nodes >= np.array(c.xLo) + 6 * c.dx) & (c.nodes <= hi - 6 * c.dx)).all()


ADVECT_CASES = ([f"synth-post-{k}" for k in POST_PASSES]
                + ["cells-%s-%s" % ("x".join(map(str, g)), m) for g in CELL_GRIDS for m in CELL_MASKS]
                + ["cells-13x11x9-negated", "cells-13x11x9-nan", "special-13x11x9", "special-13x11x9-negated", "threshold-13x11x9",
                   "sphere-131x127x140"])


# ------------------------------------------------------------------------------------------------ narrowBand
NB_DXS = (0.05, 2.0 / 42.0, 0.1, 1.0 / 3.0)
NB_GRIDS = [(70, 21, 45), BIG_NPTS]


def threshold_field(dx):
    """A (6, 5, 4) field holding, for t = 4.1*dx and 8.1*dx (the products narrowBand forms), +-t and its two neighbours in double,
    +-0.0, NaN, +-inf, and ordinary values on both sides of each threshold."""
    vals = []
    for t in (4.1 * dx, 8.1 * dx):
        for v in (t, np.nextafter(t, 0.0), np.nextafter(t, np.inf)):
            vals += [v, -v]
    vals += [0.0, -0.0, np.nan, np.inf, -np.inf]
    rng = np.random.default_rng(9)
    vals += list(rng.uniform(-12.0, 12.0, 120 - len(vals)) * dx)
    return np.asfortranarray(np.array(vals).reshape((6, 5, 4), order="F"))


def nb_phi(npts):
    """the field of the non-cubic narrowBand comparisons"""
    if npts == BIG_NPTS:
        return big_phi()[0], BIG_DX
    from levelsetfortran_amd import fields

    return fields.sphere_phi0(npts, radius=0.7, centers=((0.1, -0.2, 0.05),))


def same_bits(a, b):
    """equal as bit patterns: NaN equals NaN, -0.0 differs from 0.0"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(np.int64) == b.view(np.int64)).all())
