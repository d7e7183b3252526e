"""lsf_reinit_band without a GPU: the interface through every layer (header, bindings, Python, Fortran shim), argument
validation before the library, and the sanity of the CPU emulator (tests/band_emulator.py) that the GPU tests compare with."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def _header():
    txt = open(os.path.join(ROOT, "include", "lsf.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_interface_exists_in_every_layer():
    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib, levelset

    hdr = _header()
    for name in ("lsf_reinit_band", "lsf_reinit_band_device"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    assert len(_lib.SIGNATURES["lsf_reinit_band"][1]) == 13 and len(_lib.SIGNATURES["lsf_reinit_band_device"][1]) == 15
    assert callable(lsf.reinitBand) and "reinitBand" in levelset.__all__
    assert _lib.load().lsf_version() == 106 and lsf.__version__ == "0.1.6"  # an addition: neither version moves


def test_argument_validation_happens_before_the_library():
    import levelsetfortran_amd as lsf

    phi = np.ones((6, 6, 6), order="F")
    mask = np.ones((6, 6, 6), dtype=np.int32, order="F")
    with pytest.raises(TypeError):
        lsf.reinitBand(phi, mask.astype(np.float64), 5, 5, 5, 0, 0.1, 0.01)
    with pytest.raises(ValueError):
        lsf.reinitBand(phi, np.ones((6, 6, 5), dtype=np.int32, order="F"), 5, 5, 5, 0, 0.1, 0.01)
    with pytest.raises(ValueError):
        lsf.reinitBand(np.ones((6, 6, 5), order="F"), mask, 5, 5, 5, 0, 0.1, 0.01)
    with pytest.raises(ValueError):
        lsf.reinitBand(phi, mask, 5, 5, 5, 0, 0.1, 0.01, phiS=phi.copy(order="F"))
    with pytest.raises(KeyError):
        lsf.reinitBand(phi, mask, 5, 5, 5, 0, 0.1, 0.01, arith="exact")
    assert np.all(phi == 1.0)


def test_no_cpu_fallback_without_device():
    import levelsetfortran_amd as lsf
    from levelsetfortran_amd import _lib

    if _lib.load().lsf_device_count() > 0:
        pytest.skip("a GPU is present")
    phi = np.ones((6, 6, 6), order="F")
    mask = np.ones((6, 6, 6), dtype=np.int32, order="F")
    with pytest.raises(lsf.LsfError) as e:
        lsf.reinitBand(phi, mask, 5, 5, 5, 0, 0.1, 0.01)
    assert e.value.code == _lib.LSF_ERR_NO_DEVICE
    assert np.all(phi == 1.0) and np.all(mask == 1)


def test_fortran_shim_exports_reinitband():
    src = open(os.path.join(ROOT, "levelsetfortran_amd", "fortran", "lsf_hip.f90")).read()
    public = " ".join(re.findall(r"^PUBLIC\s*::(.*)$", src, flags=re.M))
    assert re.search(r"\breinitBand\b", public)
    assert "BIND(C,NAME='lsf_reinit_band')" in src
    assert re.search(r"^SUBROUTINE reinitBand\(phi,mask,nx,ny,nz,iter,dx,h\)", src, flags=re.M)


# ---------------------------------------------------------------------------------- the emulator itself
def _field(npts):
    from levelsetfortran_amd import fields

    phi0, dx = fields.two_sphere_phi0(npts)
    return phi0, dx, fields.reinit_step(dx), tuple(n - 1 for n in npts)


def test_emulator_with_every_interior_cell_is_the_oracles_jacobi_sweep(oracle):
    import band_emulator as be

    phi0, dx, h, (nx, ny, nz) = _field((24, 21, 19))
    want = phi0.copy(order="F")
    oracle.reinit(want, nx, ny, nz, 0, dx, h, tol=0.0, order=oracle.JACOBI)  # one sweep, then the boundary condition on the walls
    got, n, tr, nan = be.reinit_band(phi0, np.ones(phi0.shape, dtype=np.int32, order="F"), nx, ny, nz, 0, dx, h, tol=0.0)
    assert n == 1 and len(tr) == 1 and not nan
    inner = (slice(1, nx), slice(1, ny), slice(1, nz))
    assert np.array_equal(got[inner], want[inner])
    wall = np.ones(phi0.shape, dtype=bool)
    wall[inner] = False
    assert np.array_equal(got[wall], phi0[wall])  # no boundary condition: the walls keep their input values
    assert not np.array_equal(want[wall], phi0[wall])
    # mask values other than 1 are "out"
    m = np.full(phi0.shape, 2, dtype=np.int32, order="F")
    got2, n2, _, _ = be.reinit_band(phi0, m, nx, ny, nz, 3, dx, h, tol=0.0)
    assert n2 == 0 and np.array_equal(got2, phi0)


def test_emulator_continues_with_the_original_sign_field(oracle):
    import band_emulator as be

    phi0, dx, h, (nx, ny, nz) = _field((24, 21, 19))
    mask = np.asfortranarray((np.abs(phi0) < 8.1 * dx).astype(np.int32))
    whole, n, tr, _ = be.reinit_band(phi0, mask, nx, ny, nz, 19, dx, h, tol=0.0)
    first, n1, tr1, _ = be.reinit_band(phi0, mask, nx, ny, nz, 9, dx, h, tol=0.0)
    second, n2, tr2, _ = be.reinit_band(first, mask, nx, ny, nz, 9, dx, h, tol=0.0, phiS=phi0)
    assert (n, n1, n2) == (20, 10, 10)
    assert np.array_equal(second, whole) and tr1 + tr2 == tr
    M = be.list_mask(mask, nx, ny, nz)
    assert np.array_equal(whole[~M], phi0[~M]) and not np.array_equal(whole[M], phi0[M])
    # the stop rule: the first sweep whose RMS is below tol is the last
    tol = float(np.sqrt(tr[4] * tr[5]))
    _, ns, trs, _ = be.reinit_band(phi0, mask, nx, ny, nz, 19, dx, h, tol=tol)
    assert trs == tr[:ns] and trs[-1] < tol and all(v >= tol for v in trs[:-1])
