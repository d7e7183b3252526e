"""The numpy statement of lsf_cast_rays (tests/cast_ref.py, the yardstick of tests/test_gpu_cast_rays.py) pinned by itself: the hit on a
plane to rounding, the order of accuracy on a sphere, agreement of hit / grad / qval with the statement of lsf_sample_points, every
status from a named ray, the band cases, and four deliberate defects of the statement shown failing these very checks.

Figures of the final statement (printed by test_sphere_accuracy, recorded in DESIGN.md section 4.23 and include/lsf.h): phi = |x| - 0.25
on 13^3 / 25^3 / 49^3 points over [-0.5, 0.5]^3, 400 rays from |o| = 2 aimed at points within 0.2 of the centre, safety 0.9, smin 0.05,
smax 1, refine 30; largest |thit - analytic| in units of each grid's own dx:
    linear  1.39e-01 / 6.28e-02 / 3.29e-02 dx      (in units of the coarsest dx: 1.39e-01 / 3.14e-02 / 8.23e-03, ratios 4.42, 3.82)
    cubic   7.89e-03 / 1.58e-03 / 5.05e-04 dx      (                             7.89e-03 / 7.92e-04 / 1.26e-04, ratios 9.96, 6.27)
The factor the issue asks of the linear order, "at least 3, since second order would give 4", is a statement about the error as a
length: in units of each grid's own dx a second-order error halves.  The test asserts it on the error as a length.
"""
import functools

import numpy as np
import pytest

import cast_ref as C
import sample_ref as S

EPS = 2.0 ** -52
R0 = 0.25
PAR = dict(safety=0.9, smin=0.05, smax=1.0, skip=1.0, refine=30, max_steps=400)


def _axes(n):
    return [np.linspace(-0.5, 0.5, n)] * 3


@functools.lru_cache(maxsize=None)
def _sphere(n, centre=(0.0, 0.0, 0.0), r=R0):
    x, y, z = np.meshgrid(*_axes(n), indexing="ij")
    f = np.asfortranarray(np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - r)
    f.setflags(write=False)
    return f, 1.0 / (n - 1)


LO = (-0.5, -0.5, -0.5)


def _sphere_t(o, d, centre=(0.0, 0.0, 0.0), r=R0):
    """the smaller root of |o + t u - c| = r, NaN where there is none"""
    u = d / np.linalg.norm(d, axis=1)[:, None]
    oc = o - np.asarray(centre)
    b = np.einsum("ij,ij->i", oc, u)
    disc = b * b - (np.einsum("ij,ij->i", oc, oc) - r * r)
    with np.errstate(invalid="ignore"):
        return -b - np.sqrt(disc)


def _clip(o, d, shape, dx, lo, tmin=0.0, tmax=1e30):
    """[t0, t1] of the rays by the slab rule, written again (no zero components here)"""
    u = d / np.linalg.norm(d, axis=1)[:, None]
    t0, t1 = np.full(len(o), tmin), np.full(len(o), tmax)
    for A in range(3):
        a, b = (lo[A] - o[:, A]) / u[:, A], (lo[A] + (shape[A] - 1) * dx - o[:, A]) / u[:, A]
        t0, t1 = np.maximum(t0, np.minimum(a, b)), np.minimum(t1, np.maximum(a, b))
    return t0, t1


@functools.lru_cache(maxsize=None)
def _aimed_rays(count=400, seed=5, aim=0.2):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((count, 3))
    o = 2.0 * v / np.linalg.norm(v, axis=1)[:, None]
    w = rng.standard_normal((count, 3))
    target = aim * rng.random(count)[:, None] ** (1 / 3) * w / np.linalg.norm(w, axis=1)[:, None]
    d = (target - o) * (0.5 + rng.random(count))[:, None]  # any length
    return o, d


# ---------------------------------------------------------------------------------- the checks (also run with a defect switched on)
def _check_plane(defect=None):
    """phi = x - c: both interpolants reproduce it, so only rounding separates thit from (c - o_x) / u_x: a dozen roundings of
    quantities no larger than t1, against the issue's bound 1e-12 (t1 - t0)"""
    n, dx, c = 17, 1.0 / 16, 0.13
    x = np.meshgrid(*_axes(n), indexing="ij")[0]
    f = np.asfortranarray(x - c)
    rng = np.random.default_rng(2)
    o = np.stack([0.6 + rng.random(300), rng.random(300) - 0.5, rng.random(300) - 0.5], axis=1)  # beyond the +x face
    target = np.stack([np.full(300, c), 0.8 * (rng.random(300) - 0.5), 0.8 * (rng.random(300) - 0.5)], axis=1)
    d = (target - o) * 3.0
    want = (c - o[:, 0]) / (d[:, 0] / np.linalg.norm(d, axis=1))
    t0, t1 = _clip(o, d, f.shape, dx, LO)
    for order in (C.LINEAR, C.CUBIC):
        r = C.cast_rays(f, dx, LO, o, d, order=order, defect=defect, **PAR)
        assert r.info[0] == 300, r.info
        err = np.abs(r.thit - want) / (t1 - t0)
        print(f"plane, order {order}: largest |thit - analytic| / (t1 - t0) = {err.max():.3g}")
        assert np.all(err <= 1e-12)
        assert np.all(np.abs(r.hit[:, 0] - c) <= 1e-12)


def _check_zero_sample(defect=None):
    """phi = -|x - c| with c on a grid plane, a ray along +x from a grid point inside in steps of exactly one cell: the third sample
    is 0.0 exactly, a crossing by the e == 0 case alone (the field is negative on both sides); and a ray whose first reference is 0.0"""
    n, dx = 17, 1.0 / 16
    x = np.meshgrid(*_axes(n), indexing="ij")[0]
    f = np.asfortranarray(-np.abs(x - 0.125))
    o = np.array([[0.0, 0.03125, -0.0625], [0.125, 0.03125, -0.0625]])
    d = np.array([[2.0, 0.0, 0.0], [2.0, 0.0, 0.0]])
    for order in (C.LINEAR, C.CUBIC):
        r = C.cast_rays(f, dx, LO, o, d, order=order, defect=defect, safety=1.0, smin=1.0, smax=1.0, refine=0, max_steps=50)
        assert list(r.status) == [C.HIT, C.HIT], r.status
        assert list(r.thit) == [0.125, 0.0] and r.info[6] == 3 + 1 + 1 + 1 and r.info[8] == 1, (r.thit, r.info)
        # with bisections the bracket [0.0625, 0.125] keeps its right end, where e == 0
        r = C.cast_rays(f, dx, LO, o[:1], d[:1], order=order, defect=defect, safety=1.0, smin=1.0, smax=1.0, refine=8, max_steps=50)
        assert r.status[0] == C.HIT and r.thit[0] == 0.125


def _status_rays():
    """name -> (origin, direction, expected status) on the 17^3 sphere"""
    nan, inf = float("nan"), float("inf")
    return {
        "through a face": ((-1.0, 0.03, 0.02), (1.0, 0.01, -0.02), C.HIT),
        "through an edge": ((-1.0, -1.0, 0.01), (1.0, 1.0, 0.0), C.HIT),
        "through a corner": ((-1.0, -1.0, -1.0), (2.0, 2.0, 2.0), C.HIT),
        "along x inside the slabs": ((-1.0, 0.1, 0.1), (1.0, 0.0, 0.0), C.HIT),
        "along x outside a slab": ((-1.0, 0.7, 0.0), (1.0, 0.0, 0.0), C.NOGRID),
        "along x on the upper wall": ((-1.0, 0.5, 0.0), (1.0, 0.0, 0.0), C.MISS),
        "pointing away": ((-1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), C.NOGRID),
        "past the box": ((-1.0, -1.0, 0.0), (1.0, -0.1, 0.0), C.NOGRID),
        "zero direction": ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), C.BAD),
        "NaN origin": ((nan, 0.0, 0.0), (1.0, 0.0, 0.0), C.BAD),
        "NaN direction": ((-1.0, 0.0, 0.0), (1.0, nan, 0.0), C.BAD),
        "+inf origin": ((0.0, inf, 0.0), (0.0, -1.0, 0.0), C.BAD),
        "-inf direction": ((0.0, 0.0, 0.0), (0.0, 0.0, -inf), C.BAD),
        "1e300 direction": ((-1.0, 0.0, 0.0), (1e300, 0.0, 0.0), C.BAD),
        "1e300 origin": ((1e300, 0.0, 0.0), (-1.0, 0.0, 0.0), C.NOGRID),
        "begins inside the body": ((0.01, 0.02, -0.01), (0.3, -1.0, 0.2), C.HIT),
        "misses the body": ((-1.0, 0.4, 0.4), (1.0, 0.0, 0.0), C.MISS),
        "grazing": ((-1.0, R0 * 1.02, 0.0), (1.0, 0.0, 0.0), C.MISS),
    }


def _check_statuses(defect=None):
    f, dx = _sphere(17)
    cases = _status_rays()
    o = np.array([c[0] for c in cases.values()])
    d = np.array([c[1] for c in cases.values()])
    want = np.array([c[2] for c in cases.values()])
    for order in (C.LINEAR, C.CUBIC):
        r = C.cast_rays(f, dx, LO, o, d, order=order, tmax=10.0, defect=defect, **PAR)
        for name, got, w in zip(cases, r.status, want):
            assert got == w, (name, got, w)
        assert r.info[:6] == [int(np.count_nonzero(want == s)) for s in range(6)] and sum(r.info[:6]) == len(cases)
        assert r.info[8] == 1  # one ray begins inside
        names = list(cases)
        hitting = want == C.HIT
        outer = hitting & (np.arange(len(o)) != names.index("begins inside the body"))
        ana, got = _sphere_t(o[outer], d[outer]), r.thit[outer]
        assert np.all(np.abs(got - ana) < 0.25 * dx), (got, ana)  # (the figure of the accuracy test is 0.14 dx; this is a sanity check)
        inside = names.index("begins inside the body")
        u = d[inside] / np.linalg.norm(d[inside])
        assert abs(np.linalg.norm(o[inside] + r.thit[inside] * u) - R0) < 0.25 * dx  # the way out
        # outputs of the rays that are not HIT
        miss = want == C.MISS
        assert np.isnan(r.hit[~hitting]).all() and np.isnan(r.grad[~hitting]).all()
        assert np.isnan(r.thit[~hitting & ~miss]).all() and not np.isnan(r.thit[miss]).any()
        _, t1 = _clip(o[[names.index("misses the body")]] + 1e-9, d[[names.index("misses the body")]] + 1e-9, f.shape, dx, LO)
        assert abs(r.thit[names.index("misses the body")] - t1[0]) < 1e-6  # the end of the march: the far wall
        assert r.info[6] < 120 * len(cases)  # smin bounds the work next to the grazing ray


def _check_tmax_short(defect=None):
    """tmax ends the ray 0.3 dx short of the surface: the last sample is AT tmax, and thit says so"""
    f, dx = _sphere(17)
    o, d = np.array([[-1.0, 0.0, 0.0]]), np.array([[1.0, 0.0, 0.0]])
    tmax = 0.75 - 0.3 * dx
    for order in (C.LINEAR, C.CUBIC):
        r = C.cast_rays(f, dx, LO, o, d, order=order, tmax=tmax, defect=defect, safety=1.0, smin=1.0, smax=1.0, refine=20, max_steps=100)
        assert r.status[0] == C.MISS and r.thit[0] == tmax, (r.status, r.thit, tmax)
        r = C.cast_rays(f, dx, LO, o, d, order=order, tmax=0.75 + 0.3 * dx, defect=defect, safety=1.0, smin=1.0, smax=1.0, refine=20, max_steps=100)
        assert r.status[0] == C.HIT and abs(r.thit[0] - 0.75) < 0.1 * dx
        # tmin beyond the near surface: the ray starts inside and leaves through the far side
        r = C.cast_rays(f, dx, LO, o, d, order=order, tmin=1.0, tmax=3.0, defect=defect, **PAR)
        assert r.status[0] == C.HIT and abs(r.thit[0] - 1.25) < 0.1 * dx and r.info[8] == 1


def _check_entry_from_outside(defect=None):
    """400 rays from |o| = 2, every one through a wall of the box and into the body: all HIT.  The first sample sits ON a wall up to
    the rounding of o + t0*u, which is what the tolerance of the locate step is for."""
    f, dx = _sphere(13)
    o, d = _aimed_rays()
    r = C.cast_rays(f, dx, LO, o, d, order=C.LINEAR, defect=defect, **PAR)
    assert r.info[:6] == [400, 0, 0, 0, 0, 0], r.info


def _mask_case(n=33, band=4.1):
    f, dx = _sphere(n)
    return f, dx, np.asfortranarray((np.abs(f) < band * dx).astype(np.int32))


def _check_mask(defect=None):
    f, dx, mask = _mask_case(band=6.1)  # (wide enough for the cubic stencil of a point 1 dx off the surface)
    par = dict(PAR, skip=1.0)
    o, d = _aimed_rays(count=200, seed=9, aim=0.1)
    for order in (C.LINEAR, C.CUBIC):
        free = C.cast_rays(f, dx, LO, o, d, order=order, defect=defect, **par)
        band = C.cast_rays(f, dx, LO, o, d, order=order, mask=mask, defect=defect, **par)
        assert free.info[0] == 200 and band.info[0] == 200 and band.info[7] > 200 and band.info[6] < free.info[6], (free.info, band.info)
        # Rays that cross the empty space in strides reach the band at other places than the free march does, so their first
        # brackets differ; both hold the one root of the one interpolant and are bisected `refine` times, so each thit lies within
        # smax*dx / 2^refine of it: the two agree within twice that (the resolution of the refinement).  Asserted: that bound.
        res = 2.0 * par["smax"] * dx / 2.0 ** par["refine"]
        diff = np.abs(band.thit - free.thit).max()
        print(f"mask, order {order}: largest |thit(mask) - thit(free)| = {diff:.3g}, resolution bound {res:.3g}")
        assert diff <= res
        # ... and to the bit where the march is the same: rays that start on the list, 1 dx off the surface, see no gap at all
        v = o / np.linalg.norm(o, axis=1)[:, None]
        near = v * (R0 + 1.0 * dx)
        a = C.cast_rays(f, dx, LO, near, -v, order=order, defect=defect, **par)
        b = C.cast_rays(f, dx, LO, near, -v, order=order, mask=mask, defect=defect, **par)
        assert b.info[0] == 200 and b.info[7] == 0 and a.info == b.info
        for k in ("thit", "hit", "grad", "status"):
            assert np.array_equal(getattr(a, k), getattr(b, k)), k
    # rays that never meet the list: strides only, MISS, nothing of phi read
    o2 = np.array([[-1.0, 0.45, 0.44], [0.46, -1.0, -0.45]])
    d2 = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    r = C.cast_rays(f, dx, LO, o2, d2, order=C.LINEAR, mask=mask, defect=defect, **par)
    assert list(r.status) == [C.MISS, C.MISS] and r.info[6] == 0 and r.info[7] >= 2 * 32 and np.allclose(r.thit, 1.5)


def _check_hole_is_lost(defect=None):
    """a hole in the list over the surface: the ray has a reference outside, strides over the hole and meets the list again inside
    the body: the crossing lies in the gap, and the ray says LOST instead of inventing a hit"""
    f, dx, mask = _mask_case(band=6.1)
    x, y, z = np.meshgrid(*_axes(33), indexing="ij")
    hole = np.sqrt((x + R0) ** 2 + y ** 2 + z ** 2) < 1.3 * dx
    holed = mask.copy(order="F")
    holed[hole] = 0
    o, d = np.array([[-1.0, 0.004, 0.003]]), np.array([[1.0, 0.0, 0.0]])
    par = dict(PAR, skip=0.5, smax=0.5)
    for order in (C.LINEAR, C.CUBIC):
        whole = C.cast_rays(f, dx, LO, o, d, order=order, mask=mask, defect=defect, **par)
        assert whole.status[0] == C.HIT and abs(whole.thit[0] - 0.75) < 0.1 * dx
        r = C.cast_rays(f, dx, LO, o, d, order=order, mask=holed, defect=defect, **par)
        assert r.status[0] == C.LOST and np.isnan(r.thit[0]) and r.info[4] == 1 and r.info[6] > 0 and r.info[7] > 0, (r.status, r.info)
    # a one-point hole 5 cells in front of the surface and a stride that carries the ray from it into the body: the bracket spans
    # the hole, its midpoints happen to miss it, and only the gap flag knows that the list was left in between
    f, dx, mask = _mask_case(band=8.1)
    pricked = mask.copy(order="F")
    pricked[3, 16, 16] = 0
    par = dict(PAR, skip=6.5, smax=0.5)
    o = np.array([[-0.5 + 1.2 * dx, 0.004, 0.003]])  # in the second cell: on the list from the first sample
    whole = C.cast_rays(f, dx, LO, o, d, order=C.LINEAR, mask=mask, defect=defect, **par)
    assert whole.status[0] == C.HIT and abs(whole.thit[0] - 6.8 * dx) < 0.1 * dx and whole.info[7] == 0
    r = C.cast_rays(f, dx, LO, o, d, order=C.LINEAR, mask=pricked, defect=defect, **par)
    assert r.status[0] == C.LOST and r.info[4] == 1 and r.info[7] == 1, (r.status, r.info)


CHECKS = {"plane": _check_plane, "zero sample": _check_zero_sample, "statuses": _check_statuses, "tmax": _check_tmax_short,
          "entry": _check_entry_from_outside, "mask": _check_mask, "hole": _check_hole_is_lost}
EXPOSED_BY = {"no_zero_case": "zero sample", "gap_ignored": "hole", "no_clamp_to_t1": "tmax", "no_tolerance": "entry"}


@pytest.mark.parametrize("name", sorted(CHECKS))
def test_the_statement_passes(name):
    CHECKS[name]()


@pytest.mark.parametrize("defect", C.DEFECTS)
def test_a_seeded_defect_fails_a_check(defect):
    assert sorted(EXPOSED_BY) == sorted(C.DEFECTS)
    with pytest.raises(AssertionError):
        CHECKS[EXPOSED_BY[defect]](defect)


# ---------------------------------------------------------------------------------- accuracy on the sphere
def test_sphere_accuracy():
    o, d = _aimed_rays()
    ana = _sphere_t(o, d)
    fig = {}
    for order, name in ((C.LINEAR, "linear"), (C.CUBIC, "cubic")):
        for n in (13, 25, 49):
            f, dx = _sphere(n)
            r = C.cast_rays(f, dx, LO, o, d, order=order, **PAR)
            assert r.info[0] == 400, r.info
            fig[name, n] = float(np.abs(r.thit - ana).max())
        e = [fig[name, n] for n in (13, 25, 49)]
        print(f"{name}: largest |thit - analytic| = " + " / ".join(f"{v * (n - 1):.3g}" for v, n in zip(e, (13, 25, 49))) + " dx of each grid; "
              + " / ".join(f"{v * 12:.3g}" for v in e) + f" in units of the coarsest dx; ratios {e[0] / e[1]:.3g}, {e[1] / e[2]:.3g}")
    for a, b in ((13, 25), (25, 49)):
        assert fig["linear", a] / fig["linear", b] >= 3.0  # second order gives 4
        assert fig["cubic", b] < fig["linear", b]


# ---------------------------------------------------------------------------------- hit, grad, qval against the sample statement
def test_hit_grad_and_qval_are_the_sample_statement_at_the_hit():
    f, dx = _sphere(25)
    x, y, z = np.meshgrid(*_axes(25), indexing="ij")
    q = np.asfortranarray(1.25 + 0.5 * x - np.sin(2.0 * y) * (0.75 + z))
    mask = np.asfortranarray((np.abs(f) < 4.1 * dx).astype(np.int32))
    o, d = _aimed_rays()
    for order in (C.LINEAR, C.CUBIC):
        for m in (None, mask):
            r = C.cast_rays(f, dx, LO, o, d, order=order, mask=m, q=q, **PAR)
            assert r.info[0] == 400
            s = S.sample_points(f, dx, LO, r.hit, order=order, mask=m, q=q)
            assert s.info[0] == 400
            assert np.array_equal(s.grad, r.grad) and np.array_equal(s.qval, r.qval)
            u = d / np.linalg.norm(d, axis=1)[:, None]
            assert np.array_equal(r.hit, o + r.thit[:, None] * u)
            # the hit lies on the level set of the interpolant up to the refinement: |phi(hit)| <= |grad| * smax*dx / 2^refine, |grad| < 2
            assert np.all(np.abs(s.val) <= 2.0 * dx / 2.0 ** PAR["refine"])


# ---------------------------------------------------------------------------------- further named cases
def test_the_nearer_of_two_spheres_is_hit():
    n, dx = 33, 1.0 / 32
    a, _ = _sphere(n, (-0.2, 0.0, 0.0), 0.125)
    b, _ = _sphere(n, (0.2, 0.0, 0.0), 0.125)
    f = np.asfortranarray(np.minimum(a, b))
    o = np.array([[-1.0, 0.01, 0.02], [1.0, 0.01, 0.02]])
    d = np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]])
    for order in (C.LINEAR, C.CUBIC):
        r = C.cast_rays(f, dx, LO, o, d, order=order, **PAR)
        assert list(r.status) == [C.HIT, C.HIT]
        want = _sphere_t(o[:1], d[:1], (-0.2, 0.0, 0.0), 0.125)[0]
        assert abs(r.thit[0] - want) < 0.25 * dx and abs(r.thit[1] - want) < 0.25 * dx  # by symmetry
        assert r.hit[0, 0] < -0.3 and r.hit[1, 0] > 0.3


def test_max_steps_too_small_and_nan_in_phi():
    f, dx = _sphere(17)
    o, d = np.array([[-1.0, 0.01, 0.02]]), np.array([[1.0, 0.0, 0.0]])
    r = C.cast_rays(f, dx, LO, o, d, **dict(PAR, max_steps=3))
    assert r.status[0] == C.STEPS and np.isnan(r.thit[0]) and r.info[:6] == [0, 0, 0, 0, 0, 1] and r.info[6] == 4
    full = C.cast_rays(f, dx, LO, o, d, **PAR)
    assert full.status[0] == C.HIT
    steps = full.info[6] - PAR["refine"] - 1 - 1  # samples of the march after the first
    assert C.cast_rays(f, dx, LO, o, d, **dict(PAR, max_steps=steps)).status[0] == C.HIT
    assert C.cast_rays(f, dx, LO, o, d, **dict(PAR, max_steps=steps - 1)).status[0] == C.STEPS
    # a NaN in phi on the ray's way: "not > 0", so the ray from outside stops at it as at a wall, short of the surface
    bad = f.copy(order="F")
    bad[2, 8, 8] = np.nan
    for order in (C.LINEAR, C.CUBIC):
        r = C.cast_rays(bad, dx, LO, o, d, order=order, **PAR)
        assert r.status[0] == C.HIT and r.thit[0] < full.thit[0] - 2 * dx and r.info[0] == 1


def test_invalid_arguments_are_refused():
    f, dx = _sphere(13)
    o, d = _aimed_rays()
    nan, inf = float("nan"), float("inf")
    for kw in (dict(dx=0.0), dict(dx=nan), dict(xLo=(0.0, inf, 0.0)), dict(iso=nan), dict(order=2), dict(tmin=-1.0), dict(tmin=nan), dict(tmax=inf),
               dict(tmin=2.0, tmax=2.0), dict(safety=0.0), dict(safety=1.5), dict(safety=nan), dict(smin=0.0), dict(smin=inf), dict(smax=0.01),
               dict(smax=inf), dict(skip=0.0), dict(skip=nan), dict(refine=-1), dict(max_steps=0), dict(org=o[:0], dir=d[:0]), dict(dir=d[:5])):
        a = dict(dict(phi=f, dx=dx, xLo=LO, org=o, dir=d, **PAR), **kw)
        with pytest.raises(C.Invalid):
            C.cast_rays(**a)


# ---------------------------------------------------------------------------------- the ray sets of the GPU test
def test_the_ray_sets_of_the_gpu_test_are_what_they_say():
    """asserted on the statement alone: in every set of 256 rays or more at least half the rays are HIT; in the largest set every
    other status occurs -- LOST under a mask only: it takes a refused sample inside a bracket or behind a reference, and without a
    mask every sample between t0 and t1 is taken"""
    import cast_cases as K

    for inst in K.INSTANCES:
        order, hasmask, hasq = inst
        for nrays in K.NRAYS:
            w = K.want(*inst, nrays)
            assert sum(w.info[:6]) == nrays and (w.qval is not None) == hasq
            if nrays >= 256:
                assert 2 * w.info[0] >= nrays, (inst, nrays, w.info)
        w = K.want(*inst, K.NRAYS[-1])
        for s in (C.MISS, C.NOGRID, C.BAD, C.STEPS):
            assert w.info[s] >= 1, (inst, s, w.info)
        assert (w.info[C.LOST] >= 1) == hasmask and (w.info[7] > 0) == hasmask and w.info[8] > 100, (inst, w.info)
    o, d = K.rays(2037)
    assert np.isnan(o).any() and np.isnan(d).any() and np.isinf(o).any() and np.isinf(d).any() and (np.abs(d) > 1e200).any()
    assert np.count_nonzero(np.count_nonzero(d == 0.0, axis=1) == 2) > 300  # axis-parallel
    assert np.signbit(o[o == 0.0]).any() and np.signbit(d[d == 0.0]).any()  # -0.0


# ---------------------------------------------------------------------------------- the interface, without a GPU
def test_the_interface_is_there_in_every_layer():
    import os
    import re

    import levelsetfortran_amd as lsf
    from conftest import ROOT
    from levelsetfortran_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "lsf.h")).read()
    defines = dict(re.findall(r"#define (LSF_CAST_[A-Z_]+) (\d+)", hdr))
    assert len(defines) == 7
    for name, value in defines.items():
        assert getattr(_lib, name) == int(value), name
    assert (C.HIT, C.MISS, C.NOGRID, C.BAD, C.LOST, C.STEPS) == (_lib.LSF_CAST_HIT, _lib.LSF_CAST_MISS, _lib.LSF_CAST_NOGRID, _lib.LSF_CAST_BAD,
                                                                 _lib.LSF_CAST_LOST, _lib.LSF_CAST_STEPS) and C.INFO_LEN == _lib.LSF_CAST_INFO_LEN
    lib = _lib.load()
    assert hasattr(lib, "lsf_cast_rays") and hasattr(lib, "lsf_cast_rays_device") and lib.lsf_version() == 106
    assert len(_lib.SIGNATURES["lsf_cast_rays_device"][1]) == len(_lib.SIGNATURES["lsf_cast_rays"][1]) + 1 == 28
    assert callable(lsf.castRays) and lsf.CastReport._fields == ("thit", "hit", "grad", "qval", "status", "info")
    f90 = open(os.path.join(ROOT, "levelsetfortran_amd", "fortran", "lsf_hip.f90")).read()
    assert "BIND(C,NAME='lsf_cast_rays')" in f90 and "PUBLIC :: castRays" in f90


def test_python_checks_come_before_the_library():
    import levelsetfortran_amd as lsf

    f, dx = _sphere(13)
    f = np.array(f, order="F")
    o, d = (np.asfortranarray(a) for a in _aimed_rays())
    n = (12, 12, 12)
    for kw in (dict(order="quintic"), dict(tmin=-1.0), dict(tmax=float("inf")), dict(safety=0.0), dict(safety=1.1), dict(smin=0.0),
               dict(smin=1.0, smax=0.5), dict(skip=0.0), dict(refine=-1), dict(max_steps=0), dict(iso=float("nan"))):
        with pytest.raises(ValueError):
            lsf.castRays(f, *n, dx, LO, o, d, **kw)
    for args in ((f, *n, 0.0, LO, o, d), (f, *n, dx, (0.0, float("nan"), 0.0), o, d), (f, *n, dx, LO, o, d[:5]), (f, *n, dx, LO, o[:0], d[:0]),
                 (f, 0, 12, 12, dx, LO, o, d)):
        with pytest.raises(ValueError):
            lsf.castRays(*args)
    with pytest.raises(TypeError):
        lsf.castRays(f, *n, dx, LO, np.ascontiguousarray(o), d)  # C order: not the layout of surfX
    with pytest.raises(TypeError):
        lsf.castRays(f, *n, dx, LO, o, d.astype(np.float32))
