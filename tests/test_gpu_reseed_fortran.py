"""lsf_reseed_points through the Fortran wrappers (tests/fortran/host_reseed.f90, LSF_RESIDENT 0 and 2) and in the chain: the reseeded
vortex loop of tests/reseed_inputs.py through the public Python calls on the device.  Everything is compared with the numpy statement
(tests/reseed_ref.py) with `==` on the bit patterns."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import points_inputs as PI
import points_ref as P
import reseed_inputs as I
import reseed_ref as R
from conftest import ROOT
from test_gpu_reseed_points import N, _bits, _dev, lsf  # noqa: F401

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "build", "dropin", "host_reseed.exec")
NPTS, SEED = 2037, -3  # (a negative INTEGER*8: the bits of 2^64 - 3)


@pytest.fixture(scope="module")
def host_reseed_exe():
    path = os.environ.get("PATH", "") + ":/opt/rocm/bin"
    if not os.path.exists(EXE):
        fc = shutil.which("amdflang", path=path)
        if fc is None:
            pytest.skip("no amdflang: tests/fortran/host_reseed.f90 cannot be built")
        p = subprocess.run(["make", "-C", os.path.join(ROOT, "levelsetfortran_amd", "fortran"), "reseed", f"FC={fc}"],
                           env=dict(os.environ, PATH=path), text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert p.returncode == 0 and os.path.exists(EXE), p.stdout[-3000:]
    return EXE


@pytest.mark.parametrize("resident", ["0", "2"])
def test_both_calls_through_the_fortran_wrappers(lsf, host_reseed_exe, tmp_path, resident):  # noqa: F811
    """a reseed from scratch, then a top-up under the mask: the statement's bits, and the counts the wrapper prints"""
    phi, mask = I.fields()
    pts, rad = I.markers(NPTS)
    useed = SEED & 0xFFFFFFFFFFFFFFFF
    w0 = I.want(R.CUBIC, False, 0, seed=useed)
    w1 = I.want(R.CUBIC, True, NPTS, seed=useed)
    k = I.MAIN
    with open(tmp_path / "reseed_in.bin", "wb") as fh:
        fh.write(np.array([*N, NPTS, k["per_cell"], R.CUBIC, k["iters"]], np.int32).tobytes())
        fh.write(np.array([I.DX, *I.LO, k["rmin"], k["rmax"], k["band"], k["tol"]], np.float64).tobytes())
        fh.write(np.array([SEED], np.int64).tobytes())
        for a in (phi, mask, pts, rad):
            fh.write(a.tobytes(order="F"))
    env = {k_: v for k_, v in os.environ.items() if not k_.startswith("LSF_")}
    env.update(LSF_RESIDENT=resident)
    p = subprocess.run(f"ulimit -s unlimited; cd {tmp_path}; {host_reseed_exe}", shell=True, env=env, text=True, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout[-3000:]
    print(p.stdout)
    raw = open(tmp_path / "reseed_out.bin", "rb").read()
    o = 0

    def take(dtype, count, shape=None):
        nonlocal o
        a = np.frombuffer(raw, dtype, count, o)
        o += a.nbytes
        return a if shape is None else a.reshape(shape, order="F")

    n0 = int(take(np.int32, 1)[0])
    assert n0 == len(w0.rad)
    assert _bits(take(np.float64, 3 * n0, (n0, 3)), w0.pts) and _bits(take(np.float64, n0), w0.rad) and np.array_equal(take(np.int32, n0), w0.src)
    n1 = int(take(np.int32, 1)[0])
    assert n1 == len(w1.rad) and np.array_equal(take(np.int32, NPTS), w1.status)
    assert _bits(take(np.float64, 3 * n1, (n1, 3)), w1.pts) and _bits(take(np.float64, n1), w1.rad) and np.array_equal(take(np.int32, n1), w1.src)
    assert o == len(raw)
    line = " ".join(p.stdout.split())
    nums = [int(x) for x in re.findall(r"(?:markers in|kept|outside|off the band|non-finite|bad radius|far|eligible cells|candidates|accepted|"
                                       r"over-full cells|largest count|markers out)\s+(\d+)", line)]
    want = [[npts, *w.info[:9], w.info[11], w.info[12], len(w.rad)] for npts, w in ((0, w0), (NPTS, w1))]
    assert nums == want[0] + want[1], (nums, want)


def test_the_reseeded_vortex_chain_equals_the_statements_loop(lsf):  # noqa: F811
    """128 x (advectField STRICT, one step; advectPoints, one step, cubic; correctField) with reseedParticles after every 16th step on
    the device seam through the public Python calls: phi, pts, rad and every per-step info equal the statement's loop with `==`"""
    import torch

    want = I.vortex_reseed_run(16)  # (computed once per process)
    phi0, vel = PI.vortex_fields()
    n = (PI.VN - 1,) * 3
    pts, rad = P.seed_particles(phi0, PI.VDX, PI.VLO)
    fwd = tuple(_dev(a) for a in vel)
    bwd = tuple(_dev(np.asfortranarray(-a)) for a in vel)
    phi = _dev(phi0)
    dpts = torch.from_numpy(np.ascontiguousarray(np.array(pts).T)).cuda().t()
    drad = torch.from_numpy(rad.copy()).cuda()
    kw = dict(I.VORTEX, order="cubic")
    for step in range(2 * PI.VSTEPS):
        V = fwd if step < PI.VSTEPS else bwd
        lsf.advectField(phi, *n, PI.VDX, PI.VDT, 1, velocity=V, arith="strict")
        a = lsf.advectPoints(dpts, *n, PI.VDX, PI.VLO, PI.VDT, 1, velocity=V, order="cubic", scheme="rk3")
        dpts = a.pts
        c = lsf.correctField(phi, *n, PI.VDX, PI.VLO, dpts, drad, slack=1.0)
        r = None
        if (step + 1) % 16 == 0:
            rep = lsf.reseedParticles(phi, *n, PI.VDX, PI.VLO, dpts, drad, seed=step + 1, **kw)
            dpts, drad, r = rep.pts, rep.rad, rep.info
        assert (a.info, c.info, r) == want["infos"][step], (step, a.info, c.info, r, want["infos"][step])
    got = phi.cpu().numpy().reshape(phi0.shape, order="F")
    assert _bits(got, want["phi"]) and _bits(dpts.cpu().numpy(), want["pts"]) and _bits(drad.cpu().numpy(), want["rad"])
