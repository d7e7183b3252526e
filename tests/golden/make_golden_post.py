#!/usr/bin/env python3
"""Generate synth_post_37x29x23.npz FROM THE REFERENCE ITSELF: narrowBand, the order-8 gradients and the node advection of
set3d.f90:470-501 on a NON-cubic grid (nx /= ny /= nz, three different xLo).

Runs only where oracle/_ref/libref_subs.so exists (`make -C oracle ref`: the reference's subs.f90 compiled with amdflang).  The
fixture is data only -- inputs and the reference's outputs -- never reference source.

  python tests/golden/make_golden_post.py          # a few seconds; rewrites tests/golden/synth_post_37x29x23.npz
  python tests/golden/make_golden_post.py --check  # regenerates in memory and compares every array with the committed file

Through ctypes it calls the reference's narrowBand, firstDeriv (order 8) and setPhiSurf (module set_subs, all arguments by
reference) and drives them with the two loops of the main program written here: the band loop over the cells with phiSB == 1
(set3d.f90:471-479) and the pass loop in which a node moves when phiSurf(n) > 1E-13 and setPhiSurf runs again after every single move
(set3d.f90:491-501).

Input (tests/advect_nodes_inputs.py: post_input): (37, 29, 23) points, dx = 0.08, xLo = (-1.3, -1.1, -0.9); phi = distance to a
sphere plus 0.01 sin(7x) cos(5y); 1 000 seeded nodes within +-2.5 dx of the sphere.

What is undefined in the reference, and how this generator deals with it.  firstDeriv reads phi four planes below and above the cell.
A band of +-8.1 dx around any closed surface is wider than the 23 - 8 = 15 z planes that have four planes to spare on both sides,
so on this grid some band cell always reads before the first or after the last element of phi, which Fortran leaves undefined.  The
generator therefore hands the reference a phi that lies inside a larger buffer with four ZERO planes before and after it: those reads
are then defined and yield 0, which is what include/lsf.h promises for them.  It asserts that
  * no read leaves that buffer,
  * some band cells do read the zero planes, and some lie within 4 points of an x or y wall (the linear wrap into the next row),
  * no gradient that a NODE ever interpolates read a zero plane: the stored nodes are the reference's answer with no undefined read.

Stored: phi, NB, SB (int8), gradPhi, nodes_in, nodes_0 / nodes_1 / nodes_2 / nodes_1000 (the nodes after that many passes),
setphisurf_calls, moved (nodes that moved at all), passes_to_settle; and for every dx of NB_DXS the reference's masks of
threshold_field(dx) (thr<q>_NB, thr<q>_SB).
"""
from __future__ import annotations

import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libref_subs.so")
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import advect_nodes_inputs as inp  # noqa: E402


class Ref:
    """the three subroutines of module set_subs; every argument goes by reference"""

    def __init__(self):
        L = ctypes.CDLL(REF_SO)
        self.nb, self.fd, self.sps = L._QMset_subsPnarrowband, L._QMset_subsPfirstderiv, L._QMset_subsPsetphisurf
        for f, nargs in ((self.nb, 7), (self.fd, 14), (self.sps, 11)):
            f.restype, f.argtypes = None, [ctypes.c_void_p] * nargs

    @staticmethod
    def _ref(*vals):
        keep = [ctypes.c_double(v) if isinstance(v, float) else ctypes.c_int(v) for v in vals]
        return keep, [ctypes.addressof(v) for v in keep]

    def narrowband(self, phi, dx):
        nx, ny, nz = (v - 1 for v in phi.shape)
        NB, SB = (np.full(phi.shape, 7, dtype=np.int32, order="F") for _ in range(2))
        keep, (a, b, c, d) = self._ref(nx, ny, nz, float(dx))
        self.nb(a, b, c, d, phi.ctypes.data, NB.ctypes.data, SB.ctypes.data)
        return NB, SB

    def gradients(self, phi_ptr, SB, dx):
        """set3d.f90:470-479"""
        nx, ny, nz = (v - 1 for v in SB.shape)
        grad = np.zeros(SB.shape + (3,), order="F")  # set3d.f90:372
        out = (ctypes.c_double * 4)()
        i, j, k, order = (ctypes.c_int(0) for _ in range(4))
        order.value = 8
        keep, (a, b, c, d) = self._ref(nx, ny, nz, float(dx))
        o = [ctypes.addressof(out) + 8 * q for q in range(4)]
        ai, aj, ak, ao = (ctypes.addressof(v) for v in (i, j, k, order))
        for ii, jj, kk in np.argwhere(SB == 1):
            i.value, j.value, k.value = int(ii), int(jj), int(kk)
            # firstDeriv(i,j,k,nx,ny,nz,dx,phi,phiX,phiY,phiZ,order,gMM,gradPhi)
            self.fd(ai, aj, ak, a, b, c, d, phi_ptr, o[0], o[1], o[2], ao, o[3], grad.ctypes.data)
        return grad

    def advect(self, phi, grad, dx, xLo, nodes, passes):
        """set3d.f90:481-501; returns ({pass count: nodes} up to the first pass that moves nothing, setPhiSurf calls, nodes that moved,
        passes until nothing moves)"""
        nx, ny, nz = (v - 1 for v in phi.shape)
        n = nodes.shape[0]
        XX = np.array(nodes, dtype=np.float64, order="F", copy=True)
        phiSurf, gsurf, lo = np.zeros(n), np.zeros((n, 3), order="F"), np.array(xLo, dtype=np.float64)
        keep, (a, b, c, d, nn) = self._ref(nx, ny, nz, float(dx), n)
        calls = 0

        def setphisurf():
            nonlocal calls
            # setPhiSurf(xLo,nx,ny,nz,dx,phiSurf,phi,nSurfNode,surfX,gradPhiSurf,gradPhi)
            self.sps(lo.ctypes.data, a, b, c, d, phiSurf.ctypes.data, phi.ctypes.data, nn, XX.ctypes.data, gsurf.ctypes.data,
                     grad.ctypes.data)
            calls += 1

        setphisurf()
        got, moved, settle = {0: XX.copy(order="F")}, np.zeros(n, dtype=bool), None
        for k in range(1, passes + 1):
            any_move = False
            for q in range(n):
                if phiSurf[q] > 1E-13:
                    XX[q, :] = XX[q, :] + phiSurf[q] * gsurf[q, :]
                    setphisurf()
                    moved[q] = any_move = True
            got[k] = XX.copy(order="F")
            if not any_move:  # every later pass repeats the same tests on the same numbers
                settle = k - 1
                break
        return got, calls, moved, settle


def generate():
    ref = Ref()
    npts, dx, xLo = inp.POST_NPTS, inp.POST_DX, inp.POST_XLO
    phi, nodes = inp.post_input()
    sx, sxy, n = npts[0], npts[0] * npts[1], phi.size
    pad = 4 * sxy
    buf = np.zeros(n + 2 * pad)
    buf[pad:pad + n] = phi.ravel(order="F")
    padded = buf[pad:pad + n].reshape(npts, order="F")  # phi inside the buffer: the four planes on either side are zero
    assert padded.flags.f_contiguous and padded.ctypes.data == buf.ctypes.data + 8 * pad

    NB, SB = ref.narrowband(padded, dx)
    assert set(np.unique(NB)) <= {0, 1} and set(np.unique(SB)) <= {0, 1}
    ijk = np.argwhere(SB == 1)
    lin = ijk[:, 0] + sx * ijk[:, 1] + sxy * ijk[:, 2]
    assert lin.min() - 4 * sxy >= -pad and lin.max() + 4 * sxy < n + pad  # no read leaves the buffer
    reads_zero_plane = (lin - 4 * sxy < 0) | (lin + 4 * sxy >= n)
    near_xy_wall = (ijk[:, 0] < 4) | (ijk[:, 0] > npts[0] - 5) | (ijk[:, 1] < 4) | (ijk[:, 1] > npts[1] - 5)
    assert reads_zero_plane.any() and near_xy_wall.any()

    grad = ref.gradients(padded.ctypes.data, SB, dx)
    got, calls, moved, settle = ref.advect(padded, grad, dx, xLo, nodes, max(inp.POST_PASSES))
    assert settle is not None and settle < 1000
    # a node moves at most once per pass, so the per-pass snapshots are every position any node ever takes
    zero_plane = np.zeros(npts, dtype=bool)
    zero_plane[tuple(ijk[reads_zero_plane].T)] = True
    for X in got.values():
        assert inp.admissible(X, tuple(v - 1 for v in npts), dx, xLo)
        c = inp.cell_of(X, dx, xLo)
        for d in np.ndindex(2, 2, 2):
            assert not zero_plane[tuple((c + np.array(d)).T)].any()
    got = {k: got[min(k, settle)] for k in inp.POST_PASSES}
    assert 0 < moved.sum() < len(moved) and not inp.same_bits(got[1], got[2]) and not inp.same_bits(got[2], got[1000])

    out = dict(nx=npts[0] - 1, ny=npts[1] - 1, nz=npts[2] - 1, dx=dx, xLo=np.array(xLo), phi=np.asfortranarray(phi),
               NB=NB.astype(np.int8), SB=SB.astype(np.int8), gradPhi=grad, nodes_in=nodes, setphisurf_calls=calls,
               moved=int(moved.sum()), passes_to_settle=settle)
    for k, X in got.items():
        out[f"nodes_{k}"] = X
    for q, tdx in enumerate(inp.NB_DXS):
        f = inp.threshold_field(tdx)
        tnb, tsb = ref.narrowband(f, tdx)
        out[f"thr{q}_NB"], out[f"thr{q}_SB"] = tnb.astype(np.int8), tsb.astype(np.int8)
    step = np.abs(got[1000] - nodes).max()
    print(f"band cells {len(lin)} ({int(reads_zero_plane.sum())} read a zero plane, {int(near_xy_wall.sum())} within 4 points of an x/y "
          f"wall); {int(moved.sum())} of {len(moved)} nodes moved, by at most {step:.3g}; settled after {settle} passes; "
          f"{calls} setPhiSurf calls")
    return out


def main():
    out = generate()
    if "--check" in sys.argv[1:]:
        old = np.load(inp.POST_FIXTURE, allow_pickle=False)
        assert sorted(old.files) == sorted(out)
        for k in old.files:
            a, b = np.asarray(out[k]), old[k]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes(order="F") == b.tobytes(order="F"), k
        print("the committed fixture is reproduced byte for byte in every array")
        return
    np.savez_compressed(inp.POST_FIXTURE, **out)
    print("wrote", inp.POST_FIXTURE, os.path.getsize(inp.POST_FIXTURE), "bytes")


if __name__ == "__main__":
    main()
