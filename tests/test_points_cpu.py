"""The numpy statement of lsf_advect_points and lsf_correct_field (tests/points_ref.py, the yardstick of tests/test_gpu_advect_points.py
and tests/test_gpu_correct_field.py) pinned by itself: closed forms, every status from a named point, the order-free scatter, five
deliberate defects of the statement shown failing these very checks, the argument checks of the library driven without a device, and
the interface in every layer.

Figures of the statement on the vortex configuration (printed by test_vortex_markers_keep_volume, recorded in DESIGN.md section 4.24):
LeVeque's deformation field on 33^3 points, a sphere of radius 0.15 at (0.35, 0.35, 0.35), dt = dx / 4, 64 steps forward and 64 with the
velocity negated, no reinitialisation; markers from the seeding rule (16 per cell, 21 347 in all), moved with the INTERPOLATED velocity
(cubic), corrected after every step with slack 1.
    volume at the start                     0.013833
    without markers   volume 0.010747 (-22.3 %)   mean |phi - phi0| over |phi0| < 1.5 dx   0.336 dx
    with markers      volume 0.012081 (-12.7 %)                                              0.191 dx      2 385 escapes used
The recorded gap of the losses is 0.003086 - 0.001752 = 0.001334; the test asserts that the loss with markers is below the loss
without by at least half of that, both measured in the same run of the statement.
"""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import points_inputs as I
import points_ref as P
import sample_ref as S

EPS = 2.0 ** -52
RECORDED_GAP = 0.003086 - 0.001752  # the volume losses without and with markers, as recorded above


def _lin_grid(n=17):
    """17^3 points over [-0.5, 0.5]^3 (dx a binary fraction)"""
    dx = 1.0 / (n - 1)
    ax = [-0.5 + np.arange(n) * dx] * 3
    return np.meshgrid(*ax, indexing="ij"), dx, (-0.5, -0.5, -0.5)


def _const(shape, c):
    return np.asfortranarray(np.full(shape, c))


def _pts(rng, m, half=0.3):
    return np.asfortranarray((rng.random((m, 3)) - 0.5) * 2 * half)


# ---------------------------------------------------------------------------------- the checks (also run with a defect switched on)
def _check_translation(defect=None):
    """a constant velocity is an exact translation to rounding: every stage adds dt*U to numbers no larger than 1, a dozen roundings
    of at most 2^-53 per step"""
    (X, _, _), dx, lo = _lin_grid()
    U = (0.3, -0.2, 0.1)
    vel = tuple(_const(X.shape, c) for c in U)
    pts = _pts(np.random.default_rng(1), 200)
    dt, n = 0.4 * dx, 7
    for order in (P.LINEAR, P.CUBIC):
        for scheme in (P.RK3, P.EULER):
            r = P.advect_points(pts, dx, lo, dt, n, velocity=vel, order=order, scheme=scheme, defect=defect)
            assert r.info[:5] == [200, 0, 0, 0, 200 * n], r.info
            err = np.abs(r.pts - (pts + n * dt * np.asarray(U))).max()
            assert err <= 12 * n * EPS, (order, scheme, err)
            assert abs(r.cfl - dt * 0.3 / dx) <= 4 * EPS


def _check_rotation(defect=None):
    """a rigid rotation conserves the radius to third order: per step the RK3 polynomial changes it by the factor
    |1 + iz - z^2/2 - i z^3/6| = 1 - z^4/24 + O(z^6), z = omega dt, so n = T / dt steps lose T omega z^3 / 24 of it and halving dt
    divides the loss by 8; both interpolants reproduce the linear field"""
    (X, Y, _), dx, lo = _lin_grid()
    om = 2.0
    vel = (np.asfortranarray(-om * Y), np.asfortranarray(om * X), _const(X.shape, 0.0))
    pts = _pts(np.random.default_rng(2), 100, 0.25)
    r0 = np.hypot(pts[:, 0], pts[:, 1])
    T = 0.5
    loss = []
    for n in (8, 16):
        dt = T / n
        r = P.advect_points(pts, dx, lo, dt, n, velocity=vel, order=P.CUBIC, scheme=P.RK3, defect=defect)
        assert r.info[0] == 100
        rel = np.abs(np.hypot(r.pts[:, 0], r.pts[:, 1]) / r0 - 1.0).max()
        z = om * dt
        assert rel <= 1.5 * n * z ** 4 / 24, (n, rel, n * z ** 4 / 24)
        loss.append(rel)
    assert loss[0] / loss[1] > 7.0, loss


def _check_radial(defect=None):
    """speed = 1 on the distance to a sphere moves a point radially by nsteps * dt: k = g / |g| has length 1 to rounding whatever
    the interpolant makes of g, and its direction is off the radius by no more than the gradient error of the interpolant, 8.8e-3 at
    this resolution (include/lsf.h, lsf_sample_points: 25^3 points, radius 0.25) -- so the radius grows by nsteps * dt * cos(theta)
    with 1 - cos(theta) <= 4e-5, and a sideways drift of nsteps * dt * theta adds its square over 2r: below 1e-4 nsteps dt in all"""
    n = 25
    dx = 1.0 / (n - 1)
    ax = [-0.5 + np.arange(n) * dx] * 3
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    phi = np.asfortranarray(np.sqrt(X * X + Y * Y + Z * Z) - 0.25)
    rng = np.random.default_rng(3)
    v = rng.standard_normal((150, 3))
    pts = np.asfortranarray(v / np.linalg.norm(v, axis=1)[:, None] * (0.25 + (rng.random(150)[:, None] - 0.5) * 2 * dx))
    dt, ns = 0.25 * dx, 4
    r = P.advect_points(pts, dx, (-0.5,) * 3, dt, ns, speed=_const(phi.shape, 1.0), phi=phi, order=P.CUBIC, defect=defect)
    assert r.info[0] == 150
    moved = np.linalg.norm(r.pts, axis=1) - np.linalg.norm(pts, axis=1)
    assert np.abs(moved - ns * dt).max() <= 1e-4 * ns * dt, np.abs(moved - ns * dt).max() / (ns * dt)
    assert 3.0 ** -0.5 * dt / dx <= r.cfl <= dt / dx * (1 + 4 * EPS)  # the largest component of a unit vector


def _check_euler_back(defect=None):
    """dt followed by -dt under Euler on a constant field returns the start, to the rounding of one sum and one difference"""
    (X, _, _), dx, lo = _lin_grid()
    vel = tuple(_const(X.shape, c) for c in (0.7, -0.4, 0.9))
    pts = _pts(np.random.default_rng(4), 100)
    a = P.advect_points(pts, dx, lo, 0.3 * dx, 1, velocity=vel, scheme=P.EULER, defect=defect)
    b = P.advect_points(a.pts, dx, lo, -0.3 * dx, 1, velocity=vel, scheme=P.EULER, defect=defect)
    assert a.info[0] == b.info[0] == 100 and np.abs(b.pts - pts).max() <= 2 * EPS


def _check_walls_and_statuses(defect=None):
    """every status from a named point; a point that would leave keeps the position of its last completed step; every returned point
    that was INSIDE on entry lies in the grid"""
    (X, Y, Z), dx, lo = _lin_grid()
    vel = (_const(X.shape, 1.0), _const(X.shape, 0.0), _const(X.shape, 0.0))
    nan, inf = float("nan"), float("inf")
    pts = np.asfortranarray(np.array([[0.5 - 0.5 * dx, 0.0, 0.0],    # one step of 0.4 dx stays, the second leaves through the +x wall
                                      [0.5, 0.1, 0.1],               # on the wall: the first step leaves
                                      [0.0, 0.0, 0.0],               # free
                                      [nan, 0.0, 0.0], [0.0, inf, 0.0], [0.0, 0.0, -inf], [1e300, 0.0, 0.0],
                                      [0.5 + 1e-12, 0.0, 0.0]]))
    r = P.advect_points(pts, dx, lo, 0.4 * dx, 3, velocity=vel, defect=defect)
    assert list(r.status) == [P.OUTSIDE, P.OUTSIDE, P.OK] + [P.OUTSIDE] * 5, r.status
    assert abs(r.pts[0, 0] - (0.5 - 0.1 * dx)) <= 4 * EPS and r.pts[1, 0] == 0.5 and r.info[:5] == [1, 7, 0, 0, 4], (r.pts[:2], r.info)
    assert r.info[5] > 0  # next to the wall a cubic request is served linearly
    assert np.array_equal(r.pts[3:].view(np.uint64), pts[3:].view(np.uint64))  # not INSIDE on entry: returned bit for bit
    assert S.locate(r.pts[:3], X.shape, dx, lo)[0].all()
    # under Euler xn is sampled by no stage of its own step: only the test of xn keeps the point in the grid
    e = P.advect_points(pts[:3], dx, lo, 0.4 * dx, 3, velocity=vel, scheme=P.EULER, defect=defect)
    assert list(e.status) == [P.OUTSIDE, P.OUTSIDE, P.OK] and S.locate(e.pts, X.shape, dx, lo)[0].all(), (e.status, e.pts)
    assert abs(e.pts[0, 0] - (0.5 - 0.1 * dx)) <= 4 * EPS and e.info[4] == 4
    # FLAT on a constant phi with the linear interpolant (the gradient is -a + a = 0 exactly); the point does not move
    flat = P.advect_points(pts[2:3], dx, lo, 0.4 * dx, 3, speed=_const(X.shape, 1.0), phi=_const(X.shape, 0.3), order=P.LINEAR, defect=defect)
    assert list(flat.status) == [P.FLAT] and flat.info == [0, 0, 0, 1, 0, 0] and flat.cfl == 0.0 and np.array_equal(flat.pts, pts[2:3])
    # OFFBAND: a hole in the mask two cells ahead
    mask = np.ones(X.shape, np.int32)
    mask[11, 8, 8] = 0
    walk = P.advect_points(pts[2:3], dx, lo, 0.4 * dx, 10, velocity=vel, mask=mask, order=P.LINEAR, defect=defect)
    assert list(walk.status) == [P.OFFBAND] and 0 < walk.info[4] < 10 and walk.pts[0, 0] < 2 * dx
    # an inf planted in u stops the points that meet it and no others
    u = np.array(vel[0])
    u[12, 8, 8] = inf
    two = np.asfortranarray(np.array([[3.5 * dx, 0.1 * dx, 0.1 * dx], [-3.5 * dx, 0.1 * dx, 0.1 * dx]]))
    met = P.advect_points(two, dx, lo, 0.4 * dx, 1, velocity=(u, vel[1], vel[2]), order=P.LINEAR, defect=defect)
    assert list(met.status) == [P.OUTSIDE, P.OK] and np.array_equal(met.pts[0], two[0]) and met.info[4] == 1


def _check_centre_marker(defect=None):
    """one escaped marker at a cell centre rebuilds the 8 corners of its cell to s (r - sqrt(3) dx / 2) and nothing else; a marker on
    its own side, and one on the wrong side by less than its radius, are INPLACE"""
    (X, _, _), dx, lo = _lin_grid()
    for s in (1.0, -1.0):
        phi = _const(X.shape, -s * 1.0)  # the marker belongs on the other side
        r = 0.3 * dx
        c = np.array([(5 + 0.5) * dx - 0.5, (7 + 0.5) * dx - 0.5, (9 + 0.5) * dx - 0.5])
        pts = np.asfortranarray(np.array([c, c + 2 * dx, c - 3 * dx]))
        rad = np.array([s * r, -s * r, s * 2.0])  # escaped; on its own side; on the wrong side by 1 < slack * 2
        out = P.correct_field(phi, dx, lo, pts, rad, slack=1.0, defect=defect)
        assert list(out.status) == [P.ESCAPED, P.INPLACE, P.INPLACE], out.status
        want = s * (r - np.sqrt((0.5 * dx * 0.5 * dx + 0.5 * dx * 0.5 * dx) + 0.5 * dx * 0.5 * dx))
        cell = out.phi[5:7, 7:9, 9:11]
        assert np.all(cell == want) and abs(want - s * (r - np.sqrt(3.0) * dx / 2)) <= 2 * EPS * dx, (cell, want)
        rest = out.phi.copy()
        rest[5:7, 7:9, 9:11] = phi[5:7, 7:9, 9:11]
        assert np.array_equal(rest, phi) and out.info == [2, 1, 0, 0, 0, 0, 8] and out.change == abs(want - (-s * 1.0))


def _check_signed_zero(defect=None):
    """max in the total order: a candidate of +0.0 beats a grid value of -0.0, the bits change and `change` stays 0.0"""
    (X, _, _), dx, lo = _lin_grid()
    phi = _const(X.shape, -0.5)
    phi[5, 7, 9] = -0.0
    pts = np.asfortranarray(np.array([[(5 + 0.5) * dx - 0.5, 7 * dx - 0.5, 9 * dx - 0.5]]))  # half a cell along x from the -0.0
    out = P.correct_field(phi, dx, lo, pts, np.array([0.5 * dx]), slack=1.0, defect=defect)
    assert list(out.status) == [P.ESCAPED]
    assert out.phi[5, 7, 9] == 0.0 and not np.signbit(out.phi[5, 7, 9]), "+0.0 did not replace -0.0"
    assert out.phi[6, 7, 9] == 0.0 and not np.signbit(out.phi[6, 7, 9])  # the other end of the edge: +0.0 against -0.5
    assert out.info[6] == 8 and out.change == 0.5  # (the other six corners take r - d, nearer to zero than -0.5)


def _check_tie_prefers_plus(defect=None):
    """fabs(plus) <= fabs(minus) ? plus : minus -- on a tie plus wins: two markers mirrored in a grid plane where phi = +0.0 offer
    +c and -c to its four shared corners"""
    (X, _, _), dx, lo = _lin_grid()
    phi = np.asfortranarray(X - (6 * dx - 0.5))  # zero on the plane i = 6, exactly
    assert np.all(phi[6] == 0.0)
    y, z = (7 + 0.5) * dx - 0.5, (9 + 0.5) * dx - 0.5
    pts = np.asfortranarray(np.array([[(5 + 0.5) * dx - 0.5, y, z], [(6 + 0.5) * dx - 0.5, y, z]]))
    rad = np.array([dx, -dx])  # each on the wrong side; the spheres reach the corners (sqrt(3)/2 dx away)
    out = P.correct_field(phi, dx, lo, pts, rad, slack=0.0, defect=defect)
    assert list(out.status) == [P.ESCAPED, P.ESCAPED]
    c = dx - np.sqrt((0.5 * dx * 0.5 * dx + 0.5 * dx * 0.5 * dx) + 0.5 * dx * 0.5 * dx)
    assert c > 0 and np.all(out.phi[6, 7:9, 9:11] == c), out.phi[6, 7:9, 9:11]


def _check_order_free(defect=None):
    """a permutation of the particles leaves the corrected field, the counts and `change` bit-identical; status follows the particles"""
    phi, pts, rad = I.correct_inputs()
    mask = I.small_fields()[5]
    perm = np.random.default_rng(9).permutation(len(rad))
    for m in (None, mask):
        for slack in (0.0, 1.0):
            a = P.correct_field(phi, I.DX, I.LO, pts, rad, mask=m, slack=slack, defect=defect)
            b = P.correct_field(phi, I.DX, I.LO, np.asfortranarray(pts[perm]), rad[perm], mask=m, slack=slack, defect=defect)
            assert np.array_equal(a.phi.view(np.uint64), b.phi.view(np.uint64)) and a.info == b.info and a.change == b.change
            assert np.array_equal(a.status[perm], b.status)


CHECKS = {"translation": _check_translation, "rotation": _check_rotation, "radial": _check_radial, "euler back": _check_euler_back,
          "walls and statuses": _check_walls_and_statuses, "centre marker": _check_centre_marker, "signed zero": _check_signed_zero,
          "tie prefers plus": _check_tie_prefers_plus, "order free": _check_order_free}
# the named check that each deliberate defect of the statement fails
CAUGHT_BY = {"swap_025_075": "translation", "xn_not_tested": "walls and statuses", "escape_plus_r": "centre marker",
             "float_max": "signed zero", "prefer_minus": "tie prefers plus"}


@pytest.mark.parametrize("name", sorted(CHECKS))
def test_the_statement_passes(name):
    CHECKS[name]()


@pytest.mark.parametrize("defect", P.DEFECTS)
def test_a_seeded_defect_fails_a_check(defect):
    assert set(CAUGHT_BY) == set(P.DEFECTS)
    with pytest.raises(AssertionError):
        CHECKS[CAUGHT_BY[defect]](defect)


def test_three_fields_under_one_set_of_weights_equal_the_sample_statement():
    """each component of the velocity at a point is `val` of sample_ref.sample_points of that field there, bit for bit, under both
    orders, with and without the mask; so is the pair (speed, grad phi)"""
    phi, u, v, w, f, mask = I.small_fields()
    pts = I.draw_points(2037, False)
    for order in (P.LINEAR, P.CUBIC):
        for m in (None, mask):
            st, k, fb = P.rhs((u, v, w), None, None, m, I.DX, I.LO, pts, order)
            for A, field in enumerate((u, v, w)):
                want = S.sample_points(field, I.DX, I.LO, pts, order=order, mask=m)
                assert np.array_equal(st, want.status)
                ok = st == P.OK
                assert np.array_equal(k[ok, A].view(np.uint64), want.val[ok].view(np.uint64))
            assert fb.sum() == S.sample_points(u, I.DX, I.LO, pts, order=order, mask=m).info[3]
            st, k, _ = P.rhs(None, f, phi, m, I.DX, I.LO, pts, order)
            want = S.sample_points(phi, I.DX, I.LO, pts, order=order, mask=m, q=f)
            g = want.grad
            with np.errstate(all="ignore"):
                nrm = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
                ok = st == P.OK
                for A in range(3):
                    assert np.array_equal(k[ok, A].view(np.uint64), ((want.qval * g[:, A]) / nrm)[ok].view(np.uint64))


def test_the_key_transform_is_the_total_order():
    x = np.array([-np.inf, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, np.inf])
    k = P.to_key(x)
    assert np.all(k[1:] > k[:-1]) and np.array_equal(P.from_key(k).view(np.uint64), x.view(np.uint64))


def test_invalid_arguments_are_refused_by_the_statement():
    (X, _, _), dx, lo = _lin_grid(5)
    one = _const(X.shape, 1.0)
    pts = np.zeros((3, 3), order="F")
    ok = dict(velocity=(one, one, one))
    for kw in (dict(velocity=None), dict(velocity=(one, one, None)), dict(speed=one), dict(phi=one)):
        with pytest.raises(P.Invalid):
            P.advect_points(pts, dx, lo, 0.1, 1, **dict(ok, **kw))
    for args in ((pts[:0], dx, lo, 0.1, 1), (pts, 0.0, lo, 0.1, 1), (pts, dx, (0, np.nan, 0), 0.1, 1), (pts, dx, lo, np.inf, 1), (pts, dx, lo, 0.1, 0),
                 (pts, dx, lo, 0.1, P.MAX_STEPS + 1)):
        with pytest.raises(P.Invalid):
            P.advect_points(*args, **ok)
    for kw in (dict(order=2), dict(scheme=2)):
        with pytest.raises(P.Invalid):
            P.advect_points(pts, dx, lo, 0.1, 1, **dict(ok, **kw))
    rad = np.ones(3)
    for args, kw in (((one, dx, lo, pts[:0], rad[:0]), {}), ((one, -1.0, lo, pts, rad), {}), ((one, dx, lo, pts, rad), dict(slack=-1.0)),
                     ((one, dx, lo, pts, rad), dict(slack=np.nan)), ((one, dx, (np.inf, 0, 0), pts, rad), {})):
        with pytest.raises(P.Invalid):
            P.correct_field(*args, **kw)


def test_the_point_sets_of_the_gpu_tests_are_what_they_say():
    """at most 10 % of each main set ends non-OK on the statement alone (the cap of the issue; the draw was adjusted to it, see
    points_inputs.draw_points); every npts, both signs of dt and both step counts occur with and without the mask; the correction
    inputs make between a tenth and a half of the markers escape and hold every planted case"""
    cases = I.advect_cases()
    assert len(cases) == 24 and len({(c["order"], c["group"], c["masked"], c["scheme"]) for c in cases}) == 24
    for c, case in enumerate(cases):
        w = I.advect_want(c)
        assert case["npts"] - w.info[0] <= 0.10 * case["npts"], (case, w.info)
        assert sum(w.info[:4]) == case["npts"]
    assert {(c["masked"], c["nsteps"]) for c in cases} == {(m, n) for m in (False, True) for n in (1, 3)}
    assert {(c["masked"], c["npts"]) for c in cases} == {(m, n) for m in (False, True) for n in I.NPTS}
    assert {(c["scheme"], c["dt"] > 0) for c in cases} == {(s, d) for s in (P.RK3, P.EULER) for d in (False, True)}
    assert any(I.advect_want(c).info[5] > 0 for c in range(24)) and any(I.advect_want(c).info[2] > 0 for c in range(24))
    pts = I.draw_points(2037, False)
    assert np.isnan(pts).any() and np.isinf(pts).any() and (pts > 1e200).any() and not np.isnan(I.draw_points(65, False)).any()
    phi, cpts, rad = I.correct_inputs()
    assert len(rad) > 2 * 256 and np.isnan(phi).sum() == 1 and np.signbit(phi[I.ZERO_AT])
    for masked in (False, True):
        for slack in (0.0, 1.0):
            w = I.correct_want(masked, slack)
            assert 0.1 * len(rad) <= w.info[1] <= 0.5 * len(rad), w.info
            assert w.info[2] >= 18 and w.info[4] > 0 and w.info[5] == 4 and (w.info[3] > 0) == masked and sum(w.info[:6]) == len(rad)
            assert w.status[60] == P.ESCAPED and w.phi[I.ZERO_AT] == 0.0 and not np.signbit(w.phi[I.ZERO_AT])
            assert np.isnan(w.phi[I.NAN_AT]) and w.info[6] > 0


def test_vortex_markers_keep_volume():
    phi0, _ = I.vortex_fields()
    v0 = I.volume(phi0)
    plain, marked = I.vortex_run(False), I.vortex_run(True)
    va, vb = I.volume(plain["phi"]), I.volume(marked["phi"])
    ea, eb = I.band_error(plain["phi"], phi0), I.band_error(marked["phi"], phi0)
    print(f"vortex 33^3: volume at the start {v0:.6f}; without markers {va:.6f} ({100 * (va / v0 - 1):+.1f} %), mean error {ea:.3f} dx; "
          f"with {len(marked['rad'])} markers {vb:.6f} ({100 * (vb / v0 - 1):+.1f} %), mean error {eb:.3f} dx, {marked['escapes']} escapes used")
    assert all(a[0] + a[1] + a[2] + a[3] == len(marked["rad"]) for a, _ in marked["infos"])
    assert (v0 - vb) <= (v0 - va) - 0.5 * RECORDED_GAP
    assert eb < ea


# ---------------------------------------------------------------------------------- the library without a device
@functools.lru_cache(maxsize=None)
def _args_table():
    from conftest import ROOT

    src = os.path.join(ROOT, "tests", "host_args", "points_args_main.cpp")
    cxx = shutil.which("c++") or shutil.which("clang++", path="/opt/rocm/llvm/bin:/opt/rocm/bin")
    assert cxx, "no host C++ compiler (c++, or ROCm's clang++)"
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "points_args")
        subprocess.run([cxx, "-std=c++17", "-O1", "-Wno-unused-function", "-o", exe, src], check=True)
        return subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()


def test_every_refusal_through_the_args_ok_routines():
    """return code and message of every case of tests/host_args/points_args_main.cpp against the record; every refusal the header
    lists is among them, and a valid list passes"""
    from conftest import GOLDEN

    got = _args_table()
    want = open(os.path.join(GOLDEN, "points_args_messages.txt")).read().splitlines()
    assert got == want
    rows = [tuple(p.strip() for p in line.split("|")) for line in got]
    for name, rc, msg in rows:
        valid = " valid" in name or "just be" in name or "may alias" in name
        assert int(rc) == (0 if valid else 2), name
        assert (msg == "") == valid and (valid or msg.startswith("lsf_advect_points: " if name.startswith("advect") else "lsf_correct_field: ")), name
    text = "\n".join(m for _, _, m in rows)
    for needle in ("pts is NULL", "xLo is NULL", "1 of 3 given", "2 of 3 given", "neither a velocity", "speed without phi", "phi without speed",
                   "npts must be >= 1", "nx, ny, nz must be >= 1", "more than 2^31 - 1 points", "dx must be finite and > 0",
                   "xLo must hold three finite values", "dt must be finite", "unknown order", "unknown scheme", "nsteps must be in 1..4096",
                   "pts overlaps u", "pts overlaps w", "pts overlaps phi", "pts overlaps speed", "pts overlaps mask", "status overlaps pts",
                   "status overlaps v", "phi is NULL", "rad is NULL", "slack must be finite and >= 0", "phi overlaps pts", "phi overlaps rad",
                   "status overlaps phi", "status overlaps rad", "status overlaps mask"):
        assert needle in text, needle


def test_the_interface_is_there_in_every_layer():
    import levelsetfortran_amd as lsf
    from conftest import ROOT
    from levelsetfortran_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "lsf.h")).read()
    for name in ("lsf_advect_points", "lsf_advect_points_device", "lsf_correct_field", "lsf_correct_field_device"):
        assert re.search(r"\bint %s\(" % name, hdr), name
    defines = dict(re.findall(r"#define (LSF_(?:POINTS|CORRECT|ADVECT_POINTS)_[A-Z_]+) (\d+)", hdr))
    assert len(defines) == 13
    for name, value in defines.items():
        assert getattr(_lib, name) == int(value), name
    assert (P.OK, P.OUTSIDE, P.OFFBAND, P.FLAT) == (_lib.LSF_POINTS_OK, _lib.LSF_POINTS_OUTSIDE, _lib.LSF_POINTS_OFFBAND, _lib.LSF_POINTS_FLAT)
    assert (P.INPLACE, P.ESCAPED, P.C_OUTSIDE, P.C_OFFBAND, P.NONFINITE, P.BADRADIUS) == tuple(
        getattr(_lib, "LSF_CORRECT_" + n) for n in ("INPLACE", "ESCAPED", "OUTSIDE", "OFFBAND", "NONFINITE", "BADRADIUS"))
    assert (P.ADVECT_INFO_LEN, P.CORRECT_INFO_LEN, P.MAX_STEPS) == (_lib.LSF_ADVECT_POINTS_INFO_LEN, _lib.LSF_CORRECT_INFO_LEN,
                                                                    _lib.LSF_ADVECT_POINTS_MAX_STEPS)
    assert (P.RK3, P.EULER) == (_lib.LSF_ADVECT_RK3, _lib.LSF_ADVECT_EULER)
    lib = _lib.load()
    for name in ("lsf_advect_points", "lsf_advect_points_device", "lsf_correct_field", "lsf_correct_field_device"):
        assert hasattr(lib, name), name
    assert lib.lsf_version() == 106
    assert len(_lib.SIGNATURES["lsf_advect_points_device"][1]) == len(_lib.SIGNATURES["lsf_advect_points"][1]) + 1 == 21
    assert len(_lib.SIGNATURES["lsf_correct_field_device"][1]) == len(_lib.SIGNATURES["lsf_correct_field"][1]) + 1 == 15
    assert callable(lsf.advectPoints) and lsf.AdvectPointsReport._fields == ("pts", "status", "cfl", "info")
    assert callable(lsf.correctField) and lsf.CorrectReport._fields == ("status", "change", "info") and callable(lsf.seedParticles)
    f90 = open(os.path.join(ROOT, "levelsetfortran_amd", "fortran", "lsf_hip.f90")).read()
    assert "BIND(C,NAME='lsf_advect_points')" in f90 and "PUBLIC :: advectPoints" in f90
    assert "BIND(C,NAME='lsf_correct_field')" in f90 and "PUBLIC :: correctField" in f90
    csrc = os.path.join(ROOT, "levelsetfortran_amd", "csrc")
    for h in ("lsf_advect_points.hpp", "lsf_correct_field.hpp", "lsf_host_points.hpp", "lsf_host_args_points.hpp"):
        assert os.path.exists(os.path.join(csrc, h)), h


def test_python_checks_come_before_the_library():
    import levelsetfortran_amd as lsf

    phi, u, v, w, f, mask = (np.array(a, order="F") for a in I.small_fields())
    n = tuple(s - 1 for s in I.SHAPE)
    pts = np.array(I.draw_points(5, True), order="F")
    ok = dict(velocity=(u, v, w))
    for kw in (dict(order="quintic"), dict(scheme="rk4"), dict(velocity=None), dict(velocity=(u, v)), dict(speed=f), dict(phi=phi)):
        with pytest.raises(ValueError):
            lsf.advectPoints(pts, *n, I.DX, I.LO, 0.01, 1, **dict(ok, **kw))
    for args in ((pts, *n, 0.0, I.LO, 0.01, 1), (pts, *n, I.DX, (0.0, float("nan"), 0.0), 0.01, 1), (pts, *n, I.DX, I.LO, float("inf"), 1),
                 (pts, *n, I.DX, I.LO, 0.01, 0), (pts, *n, I.DX, I.LO, 0.01, 4097), (pts[:, :2], *n, I.DX, I.LO, 0.01, 1),
                 (pts[:0], *n, I.DX, I.LO, 0.01, 1), (pts, 0, n[1], n[2], I.DX, I.LO, 0.01, 1)):
        with pytest.raises(ValueError):
            lsf.advectPoints(*args, **ok)
    with pytest.raises(TypeError):
        lsf.advectPoints(np.ascontiguousarray(pts), *n, I.DX, I.LO, 0.01, 1, **ok)  # C order: not the layout of surfX
    rad = np.full(5, 0.01)
    for kw in (dict(slack=-1.0), dict(slack=float("nan"))):
        with pytest.raises(ValueError):
            lsf.correctField(phi, *n, I.DX, I.LO, pts, rad, **kw)
    with pytest.raises(ValueError):
        lsf.correctField(phi, *n, I.DX, I.LO, pts, rad[:4])
    with pytest.raises(TypeError):
        lsf.correctField(phi, *n, I.DX, I.LO, pts, rad.astype(np.float32))


def test_no_cpu_fallback_without_device():
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    if lib.lsf_device_count() > 0:
        pytest.skip("a GPU is present")
    import ctypes

    phi, u, v, w, f, mask = (np.array(a, order="F") for a in I.small_fields())
    n = tuple(s - 1 for s in I.SHAPE)
    pts = np.array(I.draw_points(5, True), order="F")
    keep = pts.copy()
    lo = np.array(I.LO)
    status, info, cfl = np.full(5, -7, np.int32), np.full(7, -7, np.int64), ctypes.c_double(-7.0)
    rc = lib.lsf_advect_points(u.ctypes.data, v.ctypes.data, w.ctypes.data, None, None, None, *n, I.DX, lo.ctypes.data, pts.ctypes.data, 5, P.CUBIC,
                               P.RK3, 0.01, 2, status.ctypes.data, ctypes.byref(cfl), info.ctypes.data)
    assert rc == _lib.LSF_ERR_NO_DEVICE and np.array_equal(pts, keep) and np.all(status == -7) and np.all(info == -7) and cfl.value == -7.0
    rad, before = np.full(5, 0.01), phi.copy()
    rc = lib.lsf_correct_field(phi.ctypes.data, None, *n, I.DX, lo.ctypes.data, pts.ctypes.data, rad.ctypes.data, 5, 1.0, status.ctypes.data,
                               ctypes.byref(cfl), info.ctypes.data)
    assert rc == _lib.LSF_ERR_NO_DEVICE and np.array_equal(phi, before) and np.all(status == -7) and np.all(info == -7) and cfl.value == -7.0
    with pytest.raises(_lib.LsfError) as e:
        __import__("levelsetfortran_amd").advectPoints(pts, *n, I.DX, I.LO, 0.01, 1, velocity=(u, v, w))
    assert e.value.code == _lib.LSF_ERR_NO_DEVICE
