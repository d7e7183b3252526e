"""lsf_redistance_band on the GPU against tests/redistance_ref.py, the serial statement of the contract in include/lsf_redistance.h:
phi -- the whole array, the bits off the list included --, passes, trace, change and the nine counts of info are compared with `==`,
on both seams.

The cases are those of tests/redistance_cases.py (its docstring says how the baseline field and mask are read;
tests/test_redistance_band_cpu.py asserts on the CPU that each case reaches the path it is named after).  Besides them: the refused
calls (a NaN at a list cell, an empty list) with phi untouched, one host-seam run under lsf_mirror 0, TRUST and TRUST | LAZY against
the device seam with phi handed on to reinitBand and curvatureBand without a sync in between, and the Fortran wrapper through
tests/fortran/host_redistance.f90."""
import os
import re
import subprocess

import numpy as np
import pytest

import redistance_cases as C
from advect_band_ref import list_of
from conftest import ROOT

pytestmark = pytest.mark.gpu

SEAMS = ["host", "device"]


@pytest.fixture(scope="module")
def lsf():
    import torch

    assert torch.cuda.is_available()
    import levelsetfortran_amd

    return levelsetfortran_amd


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a.ravel(order="F"))).cuda()  # (a copy: the shared inputs are read-only)


def _host(t, shape):
    return t.cpu().numpy().reshape(shape, order="F")


def _bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _run(lsf, seam, phi, mask, dx, **kw):
    """redistanceBand on fresh copies through one seam; returns (phi after the call, report or the error); asserts that the mask is
    unchanged"""
    n = tuple(v - 1 for v in phi.shape)
    mk = _dev if seam == "device" else (lambda a: a.copy(order="F"))
    p, m = mk(phi), mk(mask)
    back = lambda a: a if seam == "host" else _host(a, phi.shape)
    try:
        rep = lsf.redistanceBand(p, m, *n, dx, **kw)
    except lsf.LsfError as e:
        rep = e
    assert np.array_equal(back(m), mask)  # read, never written
    return back(p), rep


def _assert_equal(got, rep, want):
    differs = int(np.count_nonzero(np.ascontiguousarray(got).view(np.uint64) != np.ascontiguousarray(want.field).view(np.uint64)))
    print(f"passes {rep.passes} (want {want.passes}), trace {rep.trace}, change {rep.change!r} (want {want.change!r}), info {list(rep[4:])} "
          f"(want {want.info}); phi differs at {differs} points")
    assert differs == 0
    assert rep.passes == want.passes and rep.trace == want.trace
    assert rep.change == want.change
    assert list(rep[4:]) == want.info
    assert rep.converged == (want.trace[-1] == 0)


# ---------------------------------------------------------------------------------- 1: == the statement
@pytest.mark.parametrize("seam", SEAMS)
@pytest.mark.parametrize("case", C.CASES)
def test_equal_to_the_statement(lsf, case, seam):
    phi, mask, dx, kw = C.inputs(case)
    want = C.want(case)
    got, rep = _run(lsf, seam, phi, mask, dx, **kw)
    assert not isinstance(rep, Exception), rep
    _assert_equal(got, rep, want)
    lst = list_of(mask)
    assert _bits(got[~lst], phi[~lst])  # the list cells, and nothing else
    assert np.array_equal(got[lst] < 0, phi[lst] < 0)  # no cell changes the answer of (phi < 0)


# ---------------------------------------------------------------------------------- 2: the refused calls
@pytest.mark.parametrize("seam", SEAMS)
def test_refusals_leave_phi_untouched(lsf, seam):
    from levelsetfortran_amd import _lib

    phi, mask, dx, kw = C.inputs("baseline")
    lst = list_of(mask)
    bad = phi.copy(order="F")
    cells = np.argwhere(lst)[[5, 700, 2000]]
    bad[tuple(cells.T)] = [np.nan, np.inf, -np.inf]
    got, err = _run(lsf, seam, bad, mask, dx, **kw)
    assert isinstance(err, lsf.LsfError) and err.code == _lib.LSF_ERR_INVALID and "3 list cell(s) hold a non-finite phi" in str(err), err
    assert _bits(got, bad)
    off = bad.copy(order="F")  # ... and a non-finite value off the list is never read
    off[:] = phi
    off[~lst] = np.nan
    got, rep = _run(lsf, seam, off, mask, dx, **kw)
    assert not isinstance(rep, Exception), rep
    assert _bits(got[lst], C.want("baseline").field[lst]) and np.isnan(got[~lst]).all()
    empty = np.zeros(mask.shape, np.int32, order="F")
    empty[0, :, :] = empty[:, -1, :] = 1  # 1s on wall points only
    got, err = _run(lsf, seam, phi, empty, dx, **kw)
    assert isinstance(err, lsf.LsfError) and err.code == _lib.LSF_ERR_INVALID and "the list is empty" in str(err), err
    assert _bits(got, phi)
    got, err = _run(lsf, seam, phi, mask, dx, **dict(kw, near=1e-9))
    assert isinstance(err, lsf.LsfError) and err.code == _lib.LSF_ERR_INVALID and "no frozen cell" in str(err), err
    assert _bits(got, phi)


# ---------------------------------------------------------------------------------- 3: the host seam under lsf_mirror, and what follows
@pytest.mark.parametrize("flags", [0, 1, 3])
def test_host_chain_under_lsf_mirror(lsf, flags):
    """redistanceBand -> reinitBand -> curvatureBand on one phi and one mask through the host seam, without a sync in between, against
    the same chain through the device seam"""
    from levelsetfortran_amd import _lib, fields

    phi, mask, dx, kw = C.inputs("baseline")
    n = tuple(v - 1 for v in phi.shape)
    h = fields.reinit_step(dx)
    dp, dm, dk = _dev(phi), _dev(mask), _dev(np.zeros(phi.shape, order="F"))
    want = [lsf.redistanceBand(dp, dm, *n, dx, **kw)]
    after_first = _host(dp, phi.shape)
    assert _bits(after_first, C.want("baseline").field)
    want.append(lsf.reinitBand(dp, dm, *n, 3, dx, h, tol=0.0))
    want.append(lsf.curvatureBand(dp, dm, *n, dx, dk))
    lib = _lib.load()
    p, m, k = phi.copy(order="F"), mask.copy(order="F"), np.zeros(phi.shape, order="F")
    try:
        _lib.check(lib.lsf_mirror(flags))
        got = [lsf.redistanceBand(p, m, *n, dx, **kw)]
        if flags & _lib.LSF_MIRROR_LAZY:
            assert _bits(p, phi)  # the result lives in the twin until the host asks for it
        else:
            assert _bits(p, after_first)
        got.append(lsf.reinitBand(p, m, *n, 3, dx, h, tol=0.0))
        got.append(lsf.curvatureBand(p, m, *n, dx, k))
        _lib.check(lib.lsf_mirror_sync(p.ctypes.data))
    finally:
        _lib.check(lib.lsf_mirror(0))
        _lib.check(lib.lsf_release_workspace())
    assert got[0] == want[0]
    assert got[1].count == want[1].count and got[1].rms == want[1].rms
    assert got[2] == want[2]
    assert _bits(p, _host(dp, phi.shape)) and _bits(k, _host(dk, phi.shape)) and np.array_equal(m, mask)


# ---------------------------------------------------------------------------------- 4: the Fortran wrapper
EXE = os.path.join(ROOT, "build", "dropin", "host_redistance.exec")


@pytest.fixture(scope="module")
def host_redistance_exe():
    import shutil

    path = os.environ.get("PATH", "") + ":/opt/rocm/bin"
    if not os.path.exists(EXE):
        fc = shutil.which("amdflang", path=path)
        if fc is None:
            pytest.skip("no amdflang: tests/fortran/host_redistance.f90 cannot be built")
        p = subprocess.run(["make", "-C", os.path.join(ROOT, "levelsetfortran_amd", "fortran"), "redistance", f"FC={fc}"],
                           env=dict(os.environ, PATH=path), text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert p.returncode == 0 and os.path.exists(EXE), p.stdout[-3000:]
    return EXE


@pytest.mark.parametrize("case,resident,nml", [("baseline", "2", None), ("cap3", "0", "redist_passes = 3")])
def test_redistance_band_through_the_fortran_wrapper(lsf, host_redistance_exe, tmp_path, case, resident, nml):
    """tests/fortran/host_redistance.f90: redistanceBand of lsf_hip.f90 on a case of the statement, after a narrowBand on other arrays
    has taken the device twins: phi and the printed counts are the statement's, the mask comes back as it went in.  The pass cap of
    "cap3" reaches the call through &lsf_inputs.  resident = 2 (TRUST | LAZY) is the shim's default."""
    phi, mask, dx, kw = C.inputs(case)
    want = C.want(case)
    with open(tmp_path / "redistance_in.bin", "wb") as f:
        f.write(np.array([v - 1 for v in phi.shape], np.int32).tobytes())
        f.write(np.array([dx, kw["near"]], np.float64).tobytes())
        f.write(phi.tobytes(order="F"))
        f.write(mask.tobytes(order="F"))
    if nml:
        (tmp_path / "lsf.nml").write_text(f"&lsf_inputs\n  {nml}\n/\n")
    env = {k: v for k, v in os.environ.items() if not k.startswith("LSF_")}
    env.update(LSF_RESIDENT=resident)
    p = subprocess.run(f"ulimit -s unlimited; cd {tmp_path}; {host_redistance_exe}", shell=True, env=env, text=True, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout[-3000:]
    print(p.stdout)
    assert _bits(np.fromfile(tmp_path / "phi.bin", np.float64).reshape(phi.shape, order="F"), want.field)
    assert np.array_equal(np.fromfile(tmp_path / "mask.bin", np.int32).reshape(phi.shape, order="F"), mask)
    # (list-directed output breaks long records: the three lines are taken from their paragraph, not line by line)
    para = [q for q in (" ".join(t.split()) for t in re.split(r"\n[ \t]*\n", p.stdout)) if "Redistance on the band:" in q]
    assert len(para) == 1, p.stdout[-3000:]
    lines = para[0].split("Redistance on the band:")[1:]
    assert len(lines) == 3, p.stdout[-3000:]
    assert [int(t) for t in re.findall(r"-?\d+", lines[0])] == want.info[:4]
    assert [int(t) for t in re.findall(r"-?\d+", lines[1])] == want.info[4:]
    assert [int(t) for t in re.findall(r"-?\d+", lines[2].split("largest")[0])] == [want.passes, want.trace[-1]]
