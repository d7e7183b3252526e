"""The moving-geometry calls through the host seams under lsf_mirror, and through the Fortran shim.

Every expected value is the same call through the DEVICE seam (torch tensors) with the same arguments: those paths are pinned to the serial
statements by the test_gpu_* file of each call, and include/lsf.h promises that the two seams are equal.  Everything is compared with `==`
(fields as uint64 bit patterns), STRICT arithmetic throughout; the one exception is the parallel sum of lsf_sumsq_diff (1e-12 relative, the
allowance of test_host_seams_with_device_twins).

The inputs: the general grid (40,33,27), dx = 3/39; the body mesh_distance_ref.icosphere(2, 0.2, c) with c = the grid point (12,12,13) +
(0.3, 0.2, 0.4) dx, where the velocity advect_ref.wavy_inputs is about 0.4 of its maximum; dt at CFL 0.5.  The chain
  1 meshDistance(width 4)  2 distanceFill(band 4)  3 narrowBand  4 curvatureBand(phiNB, kappa, clamp 1)  5 q = kappa; extendFieldBand(q, phi,
  phiSB, band 1.5)  6 advectFieldBand(phi, phiSB, 2 steps)  7 evolveBand(phi, phiSB, 20 steps; RK3, core 3, ring 3, 2 sweeps, h = 0.5 dx, a
  check after every step: the parameters of the Fortran wrapper)  8 reinitBand(phi, phiSB, iter 3, h = 0.5 dx)  9 advectField(1 step)
  10 extractSurface(iso 0)
test_the_cases_are_what_the_docstring_says asserts on the serial statements (CPU): the mesh is accepted; the phiSB list after link 2 has 4 827
cells (19 chunks of 256, the last one ragged) and no cell next to a wall; the 279 frozen cells of link 5 lie in the interior phiNB list and
link 5 leaves no cell unreached; link 7 rebuilds once with no flips; no NaN anywhere.  A second grid (24,20,22) takes the slots over.

The calls that only read their mask (READERS: curvatureBand, extendFieldBand, measureBand, labelBand, distanceFill, and samplePoints /
castRays with mask=) run on the same state after link 3, their points and rays at the 162 nodes of the body; every array they write begins
with a sentinel and is compared whole, so what the arrays without a twin (kappa, gauss, q, cell_area, label) hold off the list is compared too.

What the refused calls (LSF_ERR_INVALID) of test_a_refused_call_leaves_the_unsynced_result leave behind, per call: lsf_advect_field,
lsf_advect_field_band, lsf_evolve_band, lsf_extend_field_band, lsf_curvature_band and lsf_extract_surface all keep the twins as they were,
whether the argument check or the core check refuses -- so the host array is what it was before until the sync, and the sync brings the EARLIER
un-synced result, never anything of the refused call."""
import contextlib
import ctypes
import functools
import math
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import advect_band_ref as B
import advect_ref as R
import curvature_ref as CV
import distance_fill_ref as DF
import evolve_band_ref as V
import extend_band_ref as XB
import mesh_distance_ref as M
from conftest import ROOT

pytestmark = pytest.mark.gpu

GRID, SMALL = (40, 33, 27), (24, 20, 22)
RADIUS, CENTRE_IJK, CENTRE_OFF = 0.2, (12, 12, 13), (0.3, 0.2, 0.4)
WIDTH, EXT_BAND, ADVECT_STEPS, EVOLVE_STEPS, REINIT_ITER = 4.0, 1.5, 2, 20, 3
CHUNK = 256  # MB_CH in csrc/lsf_minmax_band.hpp
SENT = dict(phi=123.0, nb=-7, sb=-9, kappa=-77.5, q=-55.25)  # what the arrays hold before the first link (tests/fortran/host_chain.f90 too)
LINKS = ["meshDistance", "distanceFill", "narrowBand", "curvatureBand", "extendFieldBand", "advectFieldBand", "evolveBand", "reinitBand",
         "advectField", "extractSurface"]
TRUST, LAZY = 1, 3  # LSF_MIRROR_TRUST, LSF_MIRROR_TRUST | LSF_MIRROR_LAZY
MODES = pytest.mark.parametrize("flags", [TRUST, LAZY], ids=["trust", "lazy"])
TRANSPORT = ["advectField", "advectFieldBand", "evolveBand"]


@pytest.fixture(scope="module")
def lsf():
    import torch

    assert torch.cuda.is_available()
    import levelsetfortran_amd

    return levelsetfortran_amd


# ------------------------------------------------------------------------------------------------ inputs and small tools
@functools.lru_cache(maxsize=None)
def _setup(npts=GRID):
    """the shared, read-only inputs of a grid"""
    from levelsetfortran_amd import fields

    x, y, z, dx = fields.grid_axes(npts)
    u, v, w, f, _ = R.wavy_inputs(npts)
    K = SimpleNamespace(npts=npts, n=tuple(m - 1 for m in npts), dx=float(dx), xlo=np.array([-1.5, -1.5, -1.5]), axes=(x, y, z), u=u, v=v, w=w)
    K.dt = 0.5 * K.dx / R.max_speed((u, v, w), None)
    K.h = 0.5 * K.dx
    if npts == GRID:
        c = tuple(float(a[i]) + o * K.dx for a, i, o in zip((x, y, z), CENTRE_IJK, CENTRE_OFF))
        X, E = M.icosphere(2, RADIUS, c)
        K.body = (np.asfortranarray(X), np.asfortranarray(E))
    for a in (u, v, w) + (K.body if npts == GRID else ()):
        a.setflags(write=False)
    return K


def _bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(a, b):
    """bit for bit: NaNs and the sign of zero included"""
    return a.dtype == b.dtype and a.shape == b.shape and bool(np.array_equal(_bits(a), _bits(b)))


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a.T, order="C")).cuda()  # (nz+1, ny+1, nx+1), i fastest: the same bytes (a copy: shared inputs are read-only)


def _home(t):
    return np.asfortranarray(t.cpu().numpy().T)


def _F(a):
    return np.array(a, order="F", copy=True)


def _fresh(npts=GRID):
    return dict(phi=np.full(npts, SENT["phi"], order="F"), nb=np.full(npts, SENT["nb"], np.int32, order="F"),
                sb=np.full(npts, SENT["sb"], np.int32, order="F"), kappa=np.full(npts, SENT["kappa"], order="F"),
                q=np.full(npts, SENT["q"], order="F"))


def _link(lsf, name, S, K):
    """one link of the chain on the arrays of S (all numpy or all CUDA tensors); returns its report as a tuple"""
    n, dx = K.n, K.dx
    vel = (S["u"], S["v"], S["w"])
    if name == "meshDistance":
        return tuple(lsf.meshDistance(S["phi"], *n, dx, K.xlo, *K.body, width=WIDTH))
    if name == "distanceFill":
        return tuple(lsf.distanceFill(S["phi"], *n, dx, band=WIDTH))
    if name == "narrowBand":
        lsf.narrowBand(*n, dx, S["phi"], S["nb"], S["sb"])
        return ()
    if name == "curvatureBand":
        return tuple(lsf.curvatureBand(S["phi"], S["nb"], *n, dx, S["kappa"], clamp=1.0))
    if name == "extendFieldBand":
        if isinstance(S["q"], np.ndarray):
            S["q"][...] = S["kappa"]  # kappa has no twin: it is home in every mode
        else:
            S["q"].copy_(S["kappa"])
        return tuple(lsf.extendFieldBand(S["q"], S["phi"], S["sb"], dx, band=EXT_BAND)[1])
    if name == "advectFieldBand":
        return tuple(lsf.advectFieldBand(S["phi"], S["sb"], *n, dx, K.dt, ADVECT_STEPS, velocity=vel))
    if name == "evolveBand":
        return tuple(lsf.evolveBand(S["phi"], S["sb"], *n, dx, K.dt, EVOLVE_STEPS, velocity=vel))
    if name == "reinitBand":
        r = lsf.reinitBand(S["phi"], S["sb"], *n, REINIT_ITER, dx, K.h, arith="strict")
        return (r.count, tuple(r.rms), r.converged)
    if name == "advectField":
        return tuple(lsf.advectField(S["phi"], *n, dx, K.dt, 1, velocity=vel))
    assert name == "extractSurface"
    sX, sE, info = lsf.extractSurface(S["phi"], *n, dx, K.xlo, iso=0.0)
    S["surfX"], S["surfElem"] = (sX, sE) if isinstance(sX, np.ndarray) else (np.asfortranarray(sX.cpu().numpy()), np.asfortranarray(sE.cpu().numpy()))
    return tuple(info)


@pytest.fixture(scope="module")
def want(lsf):
    """the chain through the device seam: after every link the report and a host copy of every array (read-only)"""
    K = _setup()
    S = {k: _dev(a) for k, a in _fresh().items()}
    S.update(u=_dev(K.u), v=_dev(K.v), w=_dev(K.w))
    out = []
    for name in LINKS:
        rep = _link(lsf, name, S, K)
        st = dict(report=rep, **{k: _home(S[k]) for k in ("phi", "nb", "sb", "kappa", "q")})
        for a in st.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        out.append(st)
    out[-1]["surfX"], out[-1]["surfElem"] = S["surfX"], S["surfElem"]
    assert all(_same(_home(S[k]), getattr(K, k)) for k in "uvw")  # read, never written
    return out


@pytest.fixture(scope="module")
def base(want):
    """the state after narrowBand (link 3), the start of the targeted cases: a distance field and its two bands"""
    st = want[LINKS.index("narrowBand")]
    return SimpleNamespace(phi=st["phi"], nb=st["nb"], sb=st["sb"])


@contextlib.contextmanager
def _mirror(flags):
    from levelsetfortran_amd import _lib

    lib = _lib.load()
    try:
        _lib.check(lib.lsf_mirror(flags))
        yield lib
    finally:
        _lib.check(lib.lsf_mirror(0))
        _lib.check(lib.lsf_release_workspace())


def _sync(lib, *arrays):
    from levelsetfortran_amd import _lib

    for a in arrays:
        _lib.check(lib.lsf_mirror_sync(a.ctypes.data))


def _transport(lsf, name, K, phi, mask, steps, velocity=None, speed=None, dt=None):
    args = (phi,) + (() if name == "advectField" else (mask,)) + (*K.n, K.dx, K.dt if dt is None else dt, steps)
    return tuple(getattr(lsf, name)(*args, velocity=velocity, speed=speed))


def _expect(lsf, name, K, phi, mask, steps, velocity=None, speed=None, dt=None):
    """a transport call through the device seam on copies: (phi, mask, report); a NaN ending gives the report ('nan', steps)"""
    p, m = _dev(phi), None if mask is None else _dev(mask)
    vel = None if velocity is None else tuple(_dev(a) for a in velocity)
    try:
        rep = _transport(lsf, name, K, p, m, steps, vel, None if speed is None else _dev(speed), dt)
    except lsf.LsfNaNError as e:
        rep = ("nan", e.report.steps)
    return _home(p), None if m is None else _home(m), rep


def _vel(K):
    return tuple(_F(a) for a in (K.u, K.v, K.w))


def _wild(mask):
    """the same list, not normalised: 5 where the mask is not 1"""
    return np.asfortranarray(np.where(mask == 1, 1, 5).astype(np.int32))


# ------------------------------------------------------------------------------------------------ the cases
@functools.lru_cache(maxsize=None)
def _statement():
    """links 1 - 7 by the serial statements, on the CPU"""
    K = _setup()
    X, E = K.body
    dx = K.dx
    P = np.stack(np.meshgrid(*K.axes, indexing="ij"), axis=-1)
    # the exact distance is needed in the tube only: points farther than (WIDTH + 1) dx from the body's bounding box are outside it
    near = ((P >= X.min(axis=0) - (WIDTH + 1) * dx) & (P <= X.max(axis=0) + (WIDTH + 1) * dx)).all(axis=-1)
    sd = np.full(GRID, np.inf)
    sd[near] = M.signed_distance(P[near], X, E)
    tubed, tube = M.clamp_columns(sd, WIDTH * dx)
    assert tube[near].sum() == tube.sum() and np.abs(sd[near]).max() > WIDTH * dx
    filled, rounds, trace, frozen = DF.fill(np.asfortranarray(tubed), dx, band=WIDTH)
    filled = np.asfortranarray(filled)
    nb = np.asfortranarray((np.abs(filled) < 4.1 * dx).astype(np.int32))
    sb = np.asfortranarray((np.abs(filled) < 8.1 * dx).astype(np.int32))
    curv = CV.curvature_band(filled, nb, dx, np.full(GRID, SENT["kappa"], order="F"), clamp=1.0)
    ext = XB.extend_band(curv.kappa.copy(order="F"), filled, sb, dx, band=EXT_BAND)
    vel = (K.u, K.v, K.w)
    adv = B.advect_band(filled, sb, vel, None, dx, K.dt, ADVECT_STEPS)
    evo = V.evolve_band(adv.field, sb, vel, None, dx, K.dt, EVOLVE_STEPS)
    return SimpleNamespace(tube=tube, fill=(filled, rounds, trace, frozen), nb=nb, sb=sb, curv=curv, ext=ext, adv=adv, evo=evo)


def test_the_cases_are_what_the_docstring_says():
    import levelsetfortran_amd as lsf  # (meshCheck is host code: this test needs no device)

    K = _setup()
    X, E = K.body
    dx = K.dx
    chk = lsf.meshCheck(X, E)
    assert chk.degenerate_triangles == 0 and chk.defective_edges == 0 and chk.signed_volume > 0  # a signed call accepts it
    assert (X.min(axis=0) > K.xlo).all() and (X.max(axis=0) < K.xlo + dx * np.array(K.n)).all()  # no triangle off the grid
    s = _statement()
    filled, rounds, trace, frozen = s.fill
    assert trace[-1] == 0 and frozen == int(s.tube.sum()) and np.isfinite(filled).all()
    lst = B.list_of(s.sb)
    assert int(lst.sum()) == 4827 == int(s.sb.sum()) and -(-4827 // CHUNK) == 19 and 4827 % CHUNK != 0
    assert not V.near_wall_of(lst).any()  # the list keeps clear of the walls
    frozen_cells = XB.frozen_of(filled, lst, dx, band=EXT_BAND)
    assert int(frozen_cells.sum()) == s.ext.frozen == 279 and not (frozen_cells & ~B.list_of(s.nb)).any()
    assert s.curv.nonfinite == 0 and np.isfinite(s.curv.kappa[B.list_of(s.nb)]).all()
    assert s.ext.unreached == 0 and s.ext.trace[-1] == 0 and np.isfinite(s.ext.field[lst]).all()
    assert not s.adv.nan and s.adv.steps == ADVECT_STEPS and s.adv.edge_flips == 0
    assert not s.evo.nan and (s.evo.steps, s.evo.rebuilds, s.evo.flips) == (EVOLVE_STEPS, 1, 0) and s.evo.entered > 0
    assert not _same(s.evo.mask, s.sb)  # the list has moved: the mask evolveBand returns is not the one it was given
    assert np.isfinite(s.evo.field).all() and abs(s.evo.cfl - 0.5) < 1e-12


def test_the_device_seam_chain_is_the_one_of_the_statements(want):
    """the expectation itself: the counts of its reports are those of the serial statements, and nothing returns NaN"""
    s = _statement()
    rep = {name: w["report"] for name, w in zip(LINKS, want)}
    print({k: v for k, v in rep.items() if k != "extendFieldBand"})
    assert rep["meshDistance"][:4] == (int(s.tube.sum()), 0, 0, 0)
    assert rep["distanceFill"][0] == s.fill[1] and rep["distanceFill"][2:] == (s.fill[3], True)
    assert rep["curvatureBand"][:3] == (s.curv.cells, s.curv.degenerate, s.curv.clamped)
    assert rep["extendFieldBand"][0] == s.ext.passes and rep["extendFieldBand"][3:] == (s.ext.cells, s.ext.frozen, s.ext.reached, 0)
    assert rep["advectFieldBand"][0] == ADVECT_STEPS and rep["advectFieldBand"][3:6] == (s.adv.cells, s.adv.edge_cells, 0)
    assert rep["evolveBand"][0] == EVOLVE_STEPS and rep["evolveBand"][3:9] == (s.evo.cells, s.evo.open_cells, 0, 1, s.evo.entered, s.evo.near_wall)
    assert rep["reinitBand"][0] == REINIT_ITER + 1 and not rep["reinitBand"][2]
    assert rep["advectField"][0] == 1 and rep["extractSurface"][0] > 0 and rep["extractSurface"][1] > 0
    for w in want[2:]:
        assert all(np.isfinite(w[k]).all() for k in ("phi", "kappa", "q"))
    assert _same(want[6]["sb"], s.evo.mask) and _same(want[2]["nb"], s.nb) and _same(want[5]["sb"], s.sb)


# ------------------------------------------------------------------------------------------------ A: the chain
@pytest.mark.parametrize("flags", [0, TRUST, LAZY], ids=["plain", "trust", "lazy"])
def test_the_chain_through_the_host_seam(lsf, want, flags):
    K = _setup()
    lazy = flags == LAZY
    first = _fresh()
    with _mirror(flags) as lib:
        S = _fresh()
        S.update(u=_F(K.u), v=_F(K.v), w=_F(K.w))
        for name, w in zip(LINKS, want):
            rep = _link(lsf, name, S, K)
            assert rep == w["report"], (name, rep, w["report"])
            for k in ("phi", "nb", "sb"):
                # LAZY: the result is on the device only and the host array is what it was before the chain began
                assert _same(S[k], first[k] if lazy else w[k]), (name, k)
            for k in ("kappa", "q"):  # no twin: home in every mode
                assert _same(S[k], w[k]), (name, k)
        assert _same(S["surfX"], want[-1]["surfX"]) and _same(S["surfElem"], want[-1]["surfElem"])
        _sync(lib, S["phi"], S["nb"], S["sb"])
        for k in ("phi", "nb", "sb"):  # phiSB: the 0/1 mask of evolveBand's final list
            assert _same(S[k], want[-1][k]), k
        assert all(_same(S[k], getattr(K, k)) for k in "uvw")


# ------------------------------------------------------------------------------------------------ 1: which twin the mask goes through
@MODES
@pytest.mark.parametrize("name", ["advectFieldBand", "evolveBand"])
def test_the_mask_goes_through_the_twin_of_the_array_it_is(lsf, base, name, flags):
    K = _setup()
    lazy = flags == LAZY
    steps = 6  # on the phiNB list (4.1 dx) evolveBand rebuilds within them
    third = np.asfortranarray(np.where(np.abs(base.phi) < 6.0 * K.dx, 1, 5).astype(np.int32))
    if name == "evolveBand":
        assert _expect(lsf, name, K, base.phi, base.nb, steps, _vel(K))[2][6] >= 1
    for which in ("nb", "sb", "third"):
        with _mirror(flags) as lib:
            S = dict(_fresh(), phi=_F(base.phi))
            vel = _vel(K)
            lsf.narrowBand(*K.n, K.dx, S["phi"], S["nb"], S["sb"])  # the twins of phiNB and phiSB: un-synced under LAZY
            mask = _F(third) if which == "third" else S[which]
            mask_in = third if which == "third" else getattr(base, which)
            want_phi, want_mask, want_rep = _expect(lsf, name, K, base.phi, mask_in, steps, vel)
            rep = _transport(lsf, name, K, S["phi"], mask, steps, vel)
            assert rep == want_rep, (which, rep, want_rep)
            other = "sb" if which == "nb" else "nb"
            if which == "third":
                # phiSB's un-synced result is home as soon as the third array takes its slot; phiNB's twin is not touched
                assert _same(S["sb"], base.sb) and _same(S["nb"], base.nb if not lazy else _fresh()["nb"])
            else:
                assert _same(S[other], getattr(base, other) if not lazy else _fresh()[other]), which  # the other twin is untouched
            if lazy:  # nothing of the call is home before its sync, the output mask of evolveBand included
                assert _same(S["phi"], base.phi) and _same(mask, third if which == "third" else _fresh()[which])
            _sync(lib, S["phi"], S["nb"], S["sb"], mask)
            assert _same(S["phi"], want_phi), which
            assert _same(mask, want_mask if name == "evolveBand" else mask_in), which
            assert _same(S[other], getattr(base, other)) and (which != "third" or _same(S["sb"], base.sb))


READERS = ["curvatureBand", "extendFieldBand", "measureBand", "labelBand", "distanceFill", "samplePoints", "castRays"]
LABEL_SENT = -7


def _rays(K):
    """points and rays at the body of the chain: its 162 nodes, and from 1.5 radii out of each node towards the centre"""
    X = K.body[0]
    c = X.mean(axis=0)
    return np.asfortranarray(X), np.asfortranarray(c + 1.5 * (X - c)), np.asfortranarray(c - X)


def _reader(lsf, name, K, phi, mask, q=None):
    """one of READERS on phi and mask (all numpy: host seam, or all CUDA tensors: device seam) with fresh inputs and outputs of its own;
    returns (what it reports, the arrays it wrote) as tuples and host arrays.  q: the second field of measureBand, samplePoints and
    castRays (default: v of the chain).  The outputs without a twin begin with a sentinel everywhere: what they hold off the list
    is part of what is compared."""
    import torch

    dev = not isinstance(phi, np.ndarray)
    mk, home = (_dev, _home) if dev else (_F, lambda a: a)
    n, dx = K.n, K.dx
    vec = (lambda a: torch.from_numpy(np.array(a.T, order="C")).cuda().t()) if dev else _F  # (npts, 3), Fortran order (a copy: the inputs are read-only)
    vhome = (lambda t: np.asfortranarray(t.cpu().numpy())) if dev else (lambda a: a)
    q = mk(K.v) if q is None else q
    if name == "curvatureBand":
        kap, ga = mk(_fresh()["kappa"]), mk(_fresh()["q"])
        return tuple(lsf.curvatureBand(phi, mask, *n, dx, kap, gauss=ga, clamp=1.0)), (home(kap), home(ga))
    if name == "extendFieldBand":
        ext = mk(K.u)
        return tuple(lsf.extendFieldBand(ext, phi, mask, dx, band=EXT_BAND)[1]), (home(ext),)
    if name == "measureBand":
        cell = mk(_fresh()["q"])
        return tuple(lsf.measureBand(phi, mask, *n, dx, K.xlo, q=q, cell_area=cell)), (home(cell),)
    if name == "labelBand":
        lab = mk(np.full(K.npts, LABEL_SENT, np.int32, order="F"))
        r = lsf.labelBand(phi, mask, *n, lab, side="both")
        return (r.ncomp, r.components.tolist(), r.passes, r.certified, r.info), (home(lab),)
    if name == "distanceFill":  # phi is in/out here: the caller compares it
        return tuple(lsf.distanceFill(phi, *n, dx, mask=mask)), ()
    pts, org, dirs = (vec(a) for a in _rays(K))
    if name == "samplePoints":
        r = lsf.samplePoints(phi, *n, dx, K.xlo, pts, mask=mask, q=q, iters=2)
    else:
        assert name == "castRays"
        r = lsf.castRays(phi, *n, dx, K.xlo, org, dirs, mask=mask, q=q)
    return r.info, tuple(vhome(a) for a in r[:-1] if a is not None)


@MODES
@pytest.mark.parametrize("name", READERS)
def test_a_read_only_mask_goes_through_the_twin_of_the_array_it_is(lsf, base, name, flags):
    """test_the_mask_goes_through_the_twin_of_the_array_it_is for the calls that only read their mask.  Every array the call writes is
    compared whole, so label, cell_area, kappa and q also keep, under lsf_mirror, what they held off the list."""
    K = _setup()
    lazy = flags == LAZY
    third = np.asfortranarray(np.where(np.abs(base.phi) < 6.0 * K.dx, 1, 5).astype(np.int32))
    phi0 = base.phi
    if name == "distanceFill":  # writes phi: beyond both bands the field is no distance any more, so that the fill has something to change
        phi0 = np.asfortranarray(np.where(np.abs(base.phi) < 8.1 * K.dx, base.phi, 1.5 * base.phi))
    for which in ("nb", "sb", "third"):
        mask_in = third if which == "third" else getattr(base, which)
        p = _dev(phi0)
        want_rep, want_out = _reader(lsf, name, K, p, _dev(mask_in))
        want_phi = _home(p)
        assert (name == "distanceFill") != _same(want_phi, phi0)  # distanceFill alone writes phi
        with _mirror(flags) as lib:
            S = dict(_fresh(), phi=_F(phi0))
            lsf.narrowBand(*K.n, K.dx, S["phi"], S["nb"], S["sb"])  # the twins of phiNB and phiSB: un-synced under LAZY
            mask = _F(third) if which == "third" else S[which]
            rep, out = _reader(lsf, name, K, S["phi"], mask)
            assert rep == want_rep, (which, rep, want_rep)
            assert len(out) == len(want_out) and all(_same(a, b) for a, b in zip(out, want_out)), which
            # the arrays without a twin: written on the list, and off the list bit for bit what they held on entry
            held = {"curvatureBand": (_fresh()["kappa"], _fresh()["q"]), "extendFieldBand": (K.u,), "measureBand": (_fresh()["q"],),
                    "labelBand": (np.full(K.npts, LABEL_SENT, np.int32, order="F"),)}.get(name, ())
            lst = B.list_of(mask_in)
            for a, h in zip(out, held):
                assert _same(a[~lst], h[~lst]) and not _same(a[lst], h[lst]), (which, name)
            other = "sb" if which == "nb" else "nb"
            if which == "third":
                # phiSB's un-synced result is home as soon as the third array takes its slot; phiNB's twin is not touched
                assert _same(S["sb"], base.sb) and _same(S["nb"], base.nb if not lazy else _fresh()["nb"])
            else:
                assert _same(S[other], getattr(base, other) if not lazy else _fresh()[other]), which  # the other twin is untouched
                assert _same(S[which], getattr(base, which) if not lazy else _fresh()[which]), which  # ... and the mask's is not written home
            assert _same(S["phi"], phi0 if lazy else want_phi)  # distanceFill's result is not home before the sync
            _sync(lib, S["phi"], S["nb"], S["sb"], mask)
            assert _same(S["phi"], want_phi), which
            assert _same(S["nb"], base.nb) and _same(S["sb"], base.sb) and _same(mask, mask_in), which  # what narrowBand made; the mask as given


# ------------------------------------------------------------------------------------------------ 2: inputs from a twin
@pytest.mark.parametrize("name", ["measureBand", "samplePoints", "castRays"])
def test_an_input_only_field_with_a_stale_host_copy_is_read_from_its_twin(lsf, base, name):
    """q of measureBand, samplePoints and castRays: under LAZY the latest content of the array lives in phi's twin slot only; the call
    reads that, and with lsf_mirror(0) it reads the host copy"""
    from levelsetfortran_amd import fields

    K = _setup()
    A0 = fields.sphere_phi0(GRID, radius=0.8)[0]
    a1 = _dev(A0)
    lsf.reinit(a1, None, None, *K.n, 1, K.dx, K.h, tol=0.0, order="jacobi", arith="strict")
    A1 = _home(a1)
    assert not _same(A1, A0) and np.isfinite(A1).all()
    want = _reader(lsf, name, K, _dev(base.phi), _dev(base.sb), q=_dev(A1))
    stale = _reader(lsf, name, K, _dev(base.phi), _dev(base.sb), q=_dev(A0))
    differs = lambda x, y: (["report"] if x[0] != y[0] else []) + [k for k, (a, b) in enumerate(zip(x[1], y[1])) if not _same(a, b)]  # which parts
    assert differs(want, stale)  # the two inputs give different results: the test bites
    with _mirror(LAZY):
        A, Bphi, m = _F(A0), _F(base.phi), _F(base.sb)
        lsf.reinit(A, None, None, *K.n, 1, K.dx, K.h, tol=0.0, order="jacobi", arith="strict")
        assert _same(A, A0)  # the host copy is stale
        got = _reader(lsf, name, K, Bphi, m, q=A)
        assert not differs(got, want), (differs(got, want), differs(got, stale), differs(want, stale))
        assert _same(A, A1)  # phi has taken the slot: A is home with the reinit result
    with _mirror(0):  # (the twins of these arrays are forgotten on the way out: their addresses will be reused)
        # without lsf_mirror the host copy is the truth: A has a current twin that holds A1, and other values on the host
        A = _F(A0)
        lsf.reinit(A, None, None, *K.n, 1, K.dx, K.h, tol=0.0, order="jacobi", arith="strict")
        assert _same(A, A1)
        A[...] = A0  # same address, same size, new content
        got = _reader(lsf, name, K, _F(base.phi), _F(base.sb), q=A)
        assert not differs(got, stale), (differs(got, stale), differs(got, want))
        assert _same(A, A0)


@pytest.mark.parametrize("name", TRANSPORT)
def test_an_input_with_a_stale_host_copy_is_read_from_its_twin(lsf, base, name):
    """the complement of test_host_inputs_are_read_from_the_host_not_from_an_earlier_twin (tests/test_gpu_advect_field.py)"""
    from levelsetfortran_amd import fields

    K = _setup()
    A0 = fields.sphere_phi0(GRID, radius=0.8)[0]
    a1 = _dev(A0)
    lsf.reinit(a1, None, None, *K.n, 1, K.dx, K.h, tol=0.0, order="jacobi", arith="strict")
    A1 = _home(a1)
    assert not _same(A1, A0) and np.isfinite(A1).all()
    mask = None if name == "advectField" else base.sb
    want_phi, want_mask, want_rep = _expect(lsf, name, K, base.phi, mask, 2, speed=A1)
    stale_phi = _expect(lsf, name, K, base.phi, mask, 2, speed=A0)[0]
    assert not _same(stale_phi, want_phi)  # the two inputs give different results: the test bites
    with _mirror(LAZY) as lib:
        A, Bphi, m = _F(A0), _F(base.phi), None if mask is None else _F(mask)
        lsf.reinit(A, None, None, *K.n, 1, K.dx, K.h, tol=0.0, order="jacobi", arith="strict")
        assert _same(A, A0)  # the host copy is stale
        rep = _transport(lsf, name, K, Bphi, m, 2, speed=A)
        assert rep == want_rep, (rep, want_rep)
        assert _same(A, A1)  # B has taken the slot: A is home with the reinit result
        assert _same(Bphi, base.phi)
        _sync(lib, Bphi, *(() if m is None else (m,)))
        assert _same(Bphi, want_phi) and (m is None or _same(m, want_mask))


# ------------------------------------------------------------------------------------------------ 3: phi as an input only
def test_calls_that_only_read_phi_read_its_twin_and_leave_it_unsynced(lsf, base):
    K = _setup()
    n, dx = K.n, K.dx
    P1 = _expect(lsf, "advectField", K, base.phi, None, 3, _vel(K))[0]

    def on_device(phi):
        p, m, kap = _dev(phi), _dev(base.sb), _dev(np.full(GRID, SENT["kappa"], order="F"))
        crep = tuple(lsf.curvatureBand(p, m, *n, dx, kap, clamp=1.0))
        q = kap.clone()
        xrep = tuple(lsf.extendFieldBand(q, p, m, dx, band=EXT_BAND)[1])
        sX, sE, info = lsf.extractSurface(p, *n, dx, K.xlo)
        return SimpleNamespace(kappa=_home(kap), crep=crep, q=_home(q), xrep=xrep, sX=np.asfortranarray(sX.cpu().numpy()),
                               sE=np.asfortranarray(sE.cpu().numpy()), info=tuple(info))

    new, old = on_device(P1), on_device(base.phi)
    # the twin and the stale host copy give different answers in every one of the three calls
    assert not _same(new.kappa, old.kappa) and not _same(new.sX, old.sX)
    q_from_old_phi = _dev(new.kappa)
    lsf.extendFieldBand(q_from_old_phi, _dev(base.phi), _dev(base.sb), dx, band=EXT_BAND)
    assert not _same(_home(q_from_old_phi), new.q)
    with _mirror(LAZY) as lib:
        S = dict(_fresh(), phi=_F(base.phi))
        lsf.narrowBand(*n, dx, S["phi"], S["nb"], S["sb"])
        lsf.advectField(S["phi"], *n, dx, K.dt, 3, velocity=_vel(K))

        def unsynced():
            return _same(S["phi"], base.phi) and _same(S["nb"], _fresh()["nb"]) and _same(S["sb"], _fresh()["sb"])

        assert unsynced()
        crep = tuple(lsf.curvatureBand(S["phi"], S["sb"], *n, dx, S["kappa"], clamp=1.0))  # the mask is phiSB: phiNB's twin is not touched
        assert crep == new.crep and _same(S["kappa"], new.kappa) and unsynced()
        S["q"][...] = S["kappa"]
        xrep = tuple(lsf.extendFieldBand(S["q"], S["phi"], S["sb"], dx, band=EXT_BAND)[1])
        assert xrep == new.xrep and _same(S["q"], new.q) and unsynced()
        sX, sE, info = lsf.extractSurface(S["phi"], *n, dx, K.xlo)
        assert tuple(info) == new.info and _same(sX, new.sX) and _same(sE, new.sE) and unsynced()
        _sync(lib, S["phi"], S["nb"], S["sb"])
        assert _same(S["phi"], P1) and _same(S["nb"], base.nb) and _same(S["sb"], base.sb)  # the twins are intact


# ------------------------------------------------------------------------------------------------ 4: the NaN path
@pytest.mark.parametrize("name", TRANSPORT)
def test_a_nan_step_stays_on_the_device_until_the_sync(lsf, base, name):
    K = _setup()
    bad = _F(base.phi)
    bad[tuple(np.argwhere(B.list_of(base.sb))[1000])] = np.nan
    mask = None if name == "advectField" else _wild(base.sb)
    want_phi, want_mask, want_rep = _expect(lsf, name, K, bad, mask, 2, _vel(K))
    assert want_rep == ("nan", 1) and np.isnan(want_phi).sum() > 1  # LSF_ERR_NAN after step 1 of 2
    with _mirror(LAZY) as lib:
        P, m = _F(bad), None if mask is None else _F(mask)
        with pytest.raises(lsf.LsfNaNError) as e:
            _transport(lsf, name, K, P, m, 2, _vel(K))
        assert e.value.report.steps == 1 and math.isnan(e.value.report.change[0])
        assert _same(P, bad) and (m is None or _same(m, mask))  # nothing is home before the sync
        _sync(lib, P, *(() if m is None else (m,)))
        assert _same(P, want_phi)
        if name == "evolveBand":
            assert _same(m, want_mask) and set(np.unique(m)) == {0, 1}
        elif m is not None:
            assert _same(m, mask)


def test_the_outputs_of_curvature_band_are_home_on_a_nan(lsf, base):
    K = _setup()
    bad = _F(base.phi)
    bad[tuple(np.argwhere(B.list_of(base.nb))[200])] = np.nan
    p, m, kap, gm = _dev(bad), _dev(base.nb), _dev(_fresh()["kappa"]), _dev(_fresh()["q"])
    with pytest.raises(lsf.LsfNaNError):
        lsf.curvatureBand(p, m, *K.n, K.dx, kap, gmag=gm, clamp=1.0)
    want_kappa, want_gmag = _home(kap), _home(gm)
    assert np.isnan(want_kappa).any() and (want_kappa[B.list_of(base.nb)] != SENT["kappa"]).all()
    with _mirror(LAZY) as lib:
        P, nb, kappa, gmag = _F(bad), _F(base.nb), _fresh()["kappa"], _fresh()["q"]
        with pytest.raises(lsf.LsfNaNError):
            lsf.curvatureBand(P, nb, *K.n, K.dx, kappa, gmag=gmag, clamp=1.0)
        assert _same(kappa, want_kappa) and _same(gmag, want_gmag)
        _sync(lib, P, nb)
        assert _same(P, bad) and _same(nb, base.nb)


# ------------------------------------------------------------------------------------------------ 5: refused calls
REFUSED = TRANSPORT + ["extendFieldBand", "curvatureBand", "extractSurface"]


@pytest.mark.parametrize("name", REFUSED)
def test_a_refused_call_leaves_the_unsynced_result(lsf, base, name):
    """LSF_ERR_INVALID by the argument check and by the core check, with an un-synced result in phi and in both masks: every one of these
    calls leaves the twins alone (see the list in the module docstring), so the sync brings the earlier result and nothing of the refused call."""
    from levelsetfortran_amd import _lib

    K = _setup()
    n, dx = K.n, K.dx
    P1 = _expect(lsf, "advectFieldBand", K, base.phi, base.sb, 1, _vel(K))[0]
    lst = B.list_of(base.sb)
    nan_u = _F(K.u)
    nan_u[tuple(np.argwhere(lst)[7])] = np.inf
    with _mirror(LAZY) as lib:
        S = dict(_fresh(), phi=_F(base.phi))
        vel = _vel(K)
        lsf.narrowBand(*n, dx, S["phi"], S["nb"], S["sb"])
        lsf.advectFieldBand(S["phi"], S["sb"], *n, dx, K.dt, 1, velocity=vel)

        def stale():
            return _same(S["phi"], base.phi) and _same(S["nb"], _fresh()["nb"]) and _same(S["sb"], _fresh()["sb"])

        assert stale()
        refused = []
        if name in TRANSPORT:
            mask = None if name == "advectField" else S["sb"]
            refused.append(lambda: _transport(lsf, name, K, S["phi"], mask, 2, vel, dt=0.0))  # the argument check
            refused.append(lambda: _transport(lsf, name, K, S["phi"], mask, 2, (nan_u, vel[1], vel[2])))  # the core check
        elif name == "extendFieldBand":
            info, done = np.zeros(4, np.int64), ctypes.c_int(0)
            trace = np.zeros(4, np.int64)
            refused.append(lambda: _lib.check(lib.lsf_extend_field_band(S["q"].ctypes.data, S["phi"].ctypes.data, S["sb"].ctypes.data, None, *n, dx,
                                                                        0.0, 8, ctypes.byref(done), trace.ctypes.data, 4, info.ctypes.data)))
            S["q"][...] = np.nan  # the frozen cells hold a non-finite q: refused by the core check, after phi and the mask were staged
            refused.append(lambda: lsf.extendFieldBand(S["q"], S["phi"], S["sb"], dx, band=EXT_BAND))
        elif name == "curvatureBand":
            info, kmax = np.zeros(4, np.int64), ctypes.c_double(0.0)
            refused.append(lambda: _lib.check(lib.lsf_curvature_band(S["phi"].ctypes.data, S["sb"].ctypes.data, S["kappa"].ctypes.data, None, None, *n,
                                                                     dx, -1.0, info.ctypes.data, ctypes.byref(kmax))))
        else:
            info, nn, nt = np.zeros(4, np.int64), ctypes.c_int(0), ctypes.c_int(0)
            refused.append(lambda: _lib.check(lib.lsf_extract_surface(S["phi"].ctypes.data, *n, 0.0, K.xlo.ctypes.data, 0.0, ctypes.byref(nn),
                                                                      ctypes.byref(nt), info.ctypes.data)))
        q_before = _F(S["q"])
        for call in refused:
            with pytest.raises(lsf.LsfError) as e:
                call()
            assert e.value.code == _lib.LSF_ERR_INVALID and not isinstance(e.value, lsf.LsfNaNError)
            assert stale() and _same(S["kappa"], _fresh()["kappa"])  # nothing is home, nothing of the refused call anywhere
        assert _same(S["q"], q_before if name != "extendFieldBand" else np.full(GRID, np.nan, order="F"))
        _sync(lib, S["phi"], S["nb"], S["sb"])
        # the earlier un-synced result, not the host copy from before it and nothing the refused call computed
        assert _same(S["phi"], P1) and _same(S["nb"], base.nb) and _same(S["sb"], base.sb)
        # a valid call follows and gives the device-seam result
        want_phi, _, want_rep = _expect(lsf, "advectFieldBand", K, P1, base.sb, 1, vel)
        assert _transport(lsf, "advectFieldBand", K, S["phi"], S["sb"], 1, vel) == want_rep
        _sync(lib, S["phi"])
        assert _same(S["phi"], want_phi)


# ------------------------------------------------------------------------------------------------ 6: nothing to do
@pytest.mark.parametrize("name,what", [(n_, w_) for n_ in TRANSPORT for w_ in ("steps = 0", "empty list") if (n_, w_) != ("advectField", "empty list")])
def test_nothing_to_do(lsf, base, name, what):
    K = _setup()
    P1 = _expect(lsf, "advectFieldBand", K, base.phi, base.sb, 1, _vel(K))[0]
    steps = 0 if what == "steps = 0" else 2
    mask = None
    if name != "advectField":
        mask = _wild(base.sb)
        if what == "empty list":  # 1 on wall points only
            mask[1:-1, 1:-1, 1:-1] = 5
            mask[0], mask[:, -1] = 1, 1
            assert (mask == 1).any() and not B.list_of(mask).any()
    _, want_mask, want_rep = _expect(lsf, name, K, P1, mask, steps, _vel(K))
    assert want_rep[0] == 0  # no step was run
    if name != "advectField":
        assert want_rep[2] == [] and (what == "steps = 0" or (want_rep[1] == 0.0 and want_rep[3] == 0 and want_rep[-1] == math.inf))
    with _mirror(LAZY) as lib:
        P, sb, m = _F(base.phi), _F(base.sb), None if mask is None else _F(mask)
        vel = _vel(K)
        lsf.advectFieldBand(P, sb, *K.n, K.dx, K.dt, 1, velocity=vel)  # an un-synced result in phi
        assert _transport(lsf, name, K, P, m, steps, vel) == want_rep
        assert _same(P, base.phi) and (m is None or _same(m, mask))
        _sync(lib, P, sb, *(() if m is None else (m,)))
        assert _same(P, P1)  # untouched: the earlier result
        if name == "evolveBand":  # in/out: normalised to 0/1, all 0 for the empty list
            assert _same(m, want_mask) and _same(m, B.list_of(mask).astype(np.int32))
        elif m is not None:
            assert _same(m, mask)


# ------------------------------------------------------------------------------------------------ 7: another grid takes the slots
@MODES
def test_a_smaller_grid_takes_the_slots_of_an_unsynced_evolve_band(lsf, base, flags):
    K, K2 = _setup(), _setup(SMALL)
    want_phi, want_mask, want_rep = _expect(lsf, "evolveBand", K, base.phi, _wild(base.sb), 3, _vel(K))
    phi2, dx2 = R.sphere_distance(SMALL, (0.0, -0.1, -0.25), 0.5)
    assert dx2 == K2.dx
    mask2 = np.asfortranarray((np.abs(phi2) < 4.1 * dx2).astype(np.int32))
    k2 = _dev(np.full(SMALL, SENT["kappa"], order="F"))
    want_crep = tuple(lsf.curvatureBand(_dev(phi2), _dev(mask2), *K2.n, dx2, k2, clamp=1.0))
    want_adv, _, want_arep = _expect(lsf, "advectField", K2, phi2, None, 1, _vel(K2))
    with _mirror(flags) as lib:
        P, m = _F(base.phi), _wild(base.sb)
        assert _transport(lsf, "evolveBand", K, P, m, 3, _vel(K)) == want_rep
        if flags == LAZY:
            assert _same(P, base.phi) and _same(m, _wild(base.sb))
        Q, mq, kq = _F(phi2), _F(mask2), np.full(SMALL, SENT["kappa"], order="F")
        assert tuple(lsf.curvatureBand(Q, mq, *K2.n, dx2, kq, clamp=1.0)) == want_crep
        assert _same(P, want_phi) and _same(m, want_mask)  # the first grid's phi and mask are home and correct
        assert _same(kq, _home(k2))
        assert _transport(lsf, "advectField", K2, Q, None, 1, _vel(K2)) == want_arep
        _sync(lib, Q, mq)
        assert _same(Q, want_adv) and _same(mq, mask2) and _same(P, want_phi) and _same(m, want_mask)


# ------------------------------------------------------------------------------------------------ 8: the host's own reads
def test_snapshot_sum_and_vti_work_on_the_twins(lsf, base, tmp_path):
    import stl_io
    from levelsetfortran_amd import _lib

    K = _setup()
    want_phi, want_mask, want_rep = _expect(lsf, "evolveBand", K, base.phi, base.sb, 5, _vel(K))
    want_sum = float(np.sum((want_phi - base.phi) ** 2))
    assert want_sum > 0.0
    with _mirror(LAZY) as lib:
        S = dict(_fresh(), phi=_F(base.phi))
        phiO = np.zeros(GRID, order="F")
        lsf.narrowBand(*K.n, K.dx, S["phi"], S["nb"], S["sb"])
        _lib.check(lib.lsf_snapshot(S["phi"].ctypes.data, phiO.ctypes.data, *K.n))
        assert _transport(lsf, "evolveBand", K, S["phi"], S["sb"], 5, _vel(K)) == want_rep
        tot = ctypes.c_double(0.0)
        _lib.check(lib.lsf_sumsq_diff(S["phi"].ctypes.data, phiO.ctypes.data, *K.n, ctypes.byref(tot)))
        assert abs(tot.value - want_sum) <= 1e-12 * want_sum, (tot.value, want_sum)
        path = str(tmp_path / "evolved.vti")
        _lib.check(lib.lsf_write_vti(path.encode(), S["phi"].ctypes.data, *K.n, K.dx, K.xlo.ctypes.data))
        assert _same(S["phi"], base.phi) and not phiO.any()  # the host arrays are still stale ...
        assert _same(np.asfortranarray(stl_io.vti_read_phi(path, GRID)), want_phi)  # ... and the file holds the device's field
        _sync(lib, S["phi"], S["sb"], phiO)
        assert _same(S["phi"], want_phi) and _same(S["sb"], want_mask) and _same(phiO, base.phi)


# ------------------------------------------------------------------------------------------------ B: a Fortran host of our own
EXE = os.path.join(ROOT, "build", "dropin", "host_chain.exec")


@pytest.fixture(scope="module")
def host_chain_exe():
    path = os.environ.get("PATH", "") + ":/opt/rocm/bin"
    if not os.path.exists(EXE):
        fc = shutil.which("amdflang", path=path)
        if fc is None:
            pytest.skip("no amdflang: tests/fortran/host_chain.f90 cannot be built")
        p = subprocess.run(["make", "-C", os.path.join(ROOT, "levelsetfortran_amd", "fortran"), "chain", f"FC={fc}"], env=dict(os.environ, PATH=path),
                           text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert p.returncode == 0 and os.path.exists(EXE), p.stdout[-3000:]
    return EXE


def _numbers(line):
    """the numbers of a list-directed line, in order"""
    return [float(t) for t in re.findall(r"[-+]?(?:\d+\.?\d*|\.\d+)(?:[EeDd][-+]?\d+)?|[-+]?Inf(?:inity)?|NaN", line)]


def _paragraph(out, head):
    """what follows `head` in the one block of output that begins with it.  Every wrapper ends its lines with an empty one, and
    list-directed output breaks a long line between two items: a block is joined before it is read."""
    hits = [p for p in (" ".join(q.split()) for q in re.split(r"\n[ \t]*\n", out)) if p.startswith(head)]
    assert len(hits) == 1, (head, hits)
    return hits[0][len(head):]


def _close(got, wanted):
    """integers exactly, reals to the 15 digits list-directed output carries (tests/test_gpu_dropin.py)"""
    assert len(got) == len(wanted), (got, wanted)
    for g, w in zip(got, wanted):
        if isinstance(w, int):
            assert g == w, (got, wanted)
        else:
            assert math.isclose(g, w, rel_tol=1e-15, abs_tol=0.0) or abs(g - w) <= 1e-15 * abs(w), (got, wanted)


@pytest.mark.parametrize("resident", ["0", "1", "2"])
def test_the_chain_through_the_fortran_wrappers(lsf, want, host_chain_exe, tmp_path, resident):
    """tests/fortran/host_chain.f90: the chain through the public wrappers of lsf_hip.f90, every array, the mesh, the STL and the printed
    lines against the device-seam chain.  resident = 2 (TRUST | LAZY) is the shim's default."""
    K = _setup()
    X, E = K.body
    with open(tmp_path / "chain_in.bin", "wb") as f:
        f.write(np.array([*K.n, X.shape[0], E.shape[0], EVOLVE_STEPS, REINIT_ITER], np.int32).tobytes())
        f.write(np.array([K.dx, *K.xlo, K.dt, WIDTH, K.h, EXT_BAND], np.float64).tobytes())
        for a in (X, E, K.u, K.v, K.w):
            f.write(a.tobytes(order="F"))
    env = {k: v for k, v in os.environ.items() if not k.startswith("LSF_")}
    env.update(LSF_ARITH="strict", LSF_RESIDENT=resident)
    p = subprocess.run(f"ulimit -s unlimited; cd {tmp_path}; {host_chain_exe}", shell=True, env=env, text=True, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout
    assert p.returncode == 0, out[-3000:]
    print(out)
    last = want[-1]
    for name, key in (("phi", "phi"), ("phiNB", "nb"), ("phiSB", "sb"), ("kappa", "kappa"), ("q", "q")):
        got = np.fromfile(tmp_path / f"{name}.bin", dtype=last[key].dtype)
        assert got.size == last[key].size and _same(got.reshape(GRID, order="F"), last[key]), name
    raw = open(tmp_path / "surf.bin", "rb").read()
    nn, nt = (int(v) for v in np.frombuffer(raw, np.int32, 2))
    assert (nn, nt) == (last["surfX"].shape[0], last["surfElem"].shape[0]) and len(raw) == 8 + 24 * nn + 12 * nt
    assert _same(np.frombuffer(raw, np.float64, 3 * nn, 8).reshape((nn, 3), order="F"), last["surfX"])
    assert _same(np.frombuffer(raw, np.int32, 3 * nt, 8 + 24 * nn).reshape((nt, 3), order="F"), last["surfElem"])
    lsf.stlWrite(str(tmp_path / "want.stl"), last["surfX"], last["surfElem"])
    assert open(tmp_path / "chain.stl", "rb").read() == open(tmp_path / "want.stl", "rb").read()
    # the printed lines of the wrappers against the reports
    rep = {name: w["report"] for name, w in zip(LINKS, want)}
    dx = K.dx
    r = rep["distanceFill"]
    _close(_numbers(_paragraph(out, "Distance fill:")), [r[0], r[2], r[1][-1]])
    r = rep["curvatureBand"]
    _close(_numbers(_paragraph(out, "Curvature on the band: list cells")), [r[0], r[1], r[2], r[3] * dx])
    r = rep["extendFieldBand"]
    _close(_numbers(_paragraph(out, "Extend field on the band:")), [r[3], r[4], r[0], r[2][-1], r[6]])
    r = rep["advectFieldBand"]  # two lines: steps, CFL, last change; list cells, edge cells, edge sign flips, margin/dx
    _close(_numbers(_paragraph(out, "Level-set transport on the band:")), [r[0], r[1], r[2][-1], r[3], r[4], r[5], r[6] / dx])
    r = rep["evolveBand"]  # steps of steps, CFL, last change; list cells, open-edge cells, sign flips, rebuilds, entered, near a wall, margin/dx
    _close(_numbers(_paragraph(out, "Band time loop:")), [r[0], EVOLVE_STEPS, r[1], r[2][-1], r[3], r[4], r[5], r[6], r[7], r[8], r[9] / dx])
    r = rep["reinitBand"]  # one line per sweep, no steady state within them
    assert not r[2] and "steady state" not in out
    _close(_numbers(_paragraph(out, "Iteration:").replace("Iteration:", "").replace("RMS Error:", "")), [x for s_ in range(r[0]) for x in (s_, r[1][s_])])
    r = rep["advectField"]
    _close(_numbers(_paragraph(out, "Level-set transport:")), [r[0], r[1], r[2][-1]])
    r = rep["extractSurface"]
    _close(_numbers(_paragraph(out, "Surface extraction:")), [r[0], r[1], r[2]])
