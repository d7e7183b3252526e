"""One statement of the Jacobi reinitialisation, two precisions -- TEST INFRASTRUCTURE.

A plain, vectorised numpy transcription of oracle/lsf_oracle.c (weno_axis with its y quirk, the first-order branch and
the :506 test, godunov, phisign, update_cell, sweep_jacobi, bc_closed, rms_change and the loop of lsf_oracle_reinit), in
the reference's textbook form and operation order: every expression is written as the C source writes it, so numpy
evaluates the same operations on the same operands, left to right, without FMA.  `dtype` picks the precision of EVERY
constant and intermediate, dx and h included (the fp32 kernels take them as `float`).

  dtype = float64   equals the C oracle's Jacobi sweep bit for bit, field and RMS trace (tests/test_reinit_f32_cpu.py):
                    that is what makes the float32 run a statement of the operation and not a second opinion.
  dtype = float32   the same statement in single precision.  Two things differ, both forced by the fp32 range:
                      * the epsilon floor of subs.f90:533-534 is 1e-30 instead of 1e-99 (include/lsf.h);
                      * the three (eps + IS_k) of a side are multiplied by one exact power of two, which puts the
                        smallest of them into [1, 2), before they are squared.  On a flat stencil eps + IS is the
                        floor, and its square (1e-60) is below the smallest fp32 number: the textbook a_k = c_k /
                        (eps+IS_k)^2 would be 1/0 and the weights inf/inf.  A power of two changes no bit of any
                        weight while the squares stay in range (the scale cancels exactly in a_k / sum a); a square
                        that now overflows gives a_k = 0, which is the limit of that weight.
                    The RMS is accumulated in float64 from the float32 differences and divided by the true product
                    nx*ny*nz (include/lsf.h "single precision"); float64 follows the oracle (INTEGER*4 product).

Nothing here is taken from the kernels' lean algebra (lsf_cell.hpp, lsf_f32.hpp).
"""
from __future__ import annotations

import numpy as np

EPS32 = float(np.finfo(np.float32).eps)


def _fmax(a, b):
    """Fortran MAX as the oracle lowers it: (a > b) ? a : b"""
    return np.where(a > b, a, b)


def _fmin(a, b):
    return np.where(a < b, a, b)


def _alphas(e0, e1, e2, T):
    """a_k = c_k / (eps + IS_k)^2, subs.f90:536-541, c = 1, 6, 3."""
    if T is np.float32:  # exact power-of-two rescale, see the module docstring
        mn = _fmin(e0, _fmin(e1, e2))
        _, ex = np.frexp(mn)
        s = np.ldexp(np.ones_like(mn), 1 - ex)
        e0, e1, e2 = e0 * s, e1 * s, e2 * s
    return T(1.) / (e0 * e0), T(6.) / (e1 * e1), T(3.) / (e2 * e2)


def weno_axis(q, dx, yquirk, T):
    """oracle weno_axis: q = seven arrays, phi at -3..+3 along the axis; returns D-, D+."""
    m3, m2, m1, c0, p1_, p2_, p3_ = q
    two, three, thirteen, seven, half = T(2.), T(3.), T(13.), T(7.), T(0.5)
    floor = T(1.E-30) if T is np.float32 else T(1.E-99)

    ap = (p3_ - two * p2_ + p1_) / dx  # :509
    am = (m3 - two * m2 + m1) / dx
    bp = (p2_ - two * p1_ + c0) / dx
    bm = (m2 - two * m1 + c0) / dx
    cp = (p1_ - two * c0 + m1) / dx  # :513
    cm = cp
    dpp = bm
    dmm = bp

    IS0p = thirteen * (ap - bp) * (ap - bp) + three * (ap - three * bp) * (ap - three * bp)  # :518
    IS0m = thirteen * (am - bm) * (am - bm) + three * (am - three * bm) * (am - three * bm)
    IS1p = thirteen * (bp - cp) * (bp - cp) + three * (bp + cp) * (bp + cp)
    IS1m = thirteen * (bm - cm) * (bm - cm) + three * (bm + cm) * (bm + cm)
    IS2p = thirteen * (cp - dpp) * (cp - dpp) + three * (three * cp - dpp) * (three * cp - dpp)
    IS2m = thirteen * (cm - dmm) * (cm - dmm) + three * (three * cm - dmm) * (three * cm - dmm)  # :523

    p0 = (m2 - m3) / dx  # :525
    p1 = (m1 - m2) / dx
    p2 = (c0 - m1) / dx
    p3 = (p1_ - c0) / dx
    p4 = (p2_ - p1_) / dx
    p5 = (p3_ - p3_) / dx if yquirk else (p3_ - p2_) / dx  # :576 / :530

    epsp = T(1.E-6) * _fmax(p1 * p1, _fmax(p2 * p2, _fmax(p3 * p3, _fmax(p4 * p4, p5 * p5)))) + floor  # :533
    epsm = T(1.E-6) * _fmax(p0 * p0, _fmax(p1 * p1, _fmax(p2 * p2, _fmax(p3 * p3, p4 * p4)))) + floor  # :534

    a0p, a1p, a2p = _alphas(epsp + IS0p, epsp + IS1p, epsp + IS2p, T)  # :536-541
    a0m, a1m, a2m = _alphas(epsm + IS0m, epsm + IS1m, epsm + IS2m, T)

    w0p = a0p / (a0p + a1p + a2p)  # :543
    w0m = a0m / (a0m + a1m + a2m)
    w2p = a2p / (a0p + a1p + a2p)
    w2m = a2m / (a0m + a1m + a2m)

    PWp = T(1.) / T(3.) * w0p * (ap - two * bp + cp) + T(1.) / T(6.) * (w2p - half) * (bp - two * cp + dpp)  # :548
    PWm = T(1.) / T(3.) * w0m * (am - two * bm + cm) + T(1.) / T(6.) * (w2m - half) * (bm - two * cm + dmm)  # :549

    cen = T(1.) / T(12.) * (-p1 + seven * p2 + seven * p3 - p4)
    return cen - PWm, cen + PWp  # :551-552


def godunov(phic, a, b, c, d, e, f, T):
    """subs.f90:667-702 from the six one-sided derivatives; returns gM."""
    z = T(0.)
    pa, pb, pc, pd, pe, pf = (_fmax(v, z) for v in (a, b, c, d, e, f))
    na, nb, nc, nd, ne, nf = (_fmin(v, z) for v in (a, b, c, d, e, f))
    pos = phic > z  # :684
    gradX = np.where(pos, _fmax(pa * pa, nb * nb), _fmax(pb * pb, na * na))
    gradY = np.where(pos, _fmax(pc * pc, nd * nd), _fmax(pd * pd, nc * nc))
    gradZ = np.where(pos, _fmax(pe * pe, nf * nf), _fmax(pf * pf, ne * ne))
    return np.sqrt(gradX + gradY + gradZ)  # :702


def phisign(pS, dxx, gM):
    return pS / np.sqrt(pS * pS + dxx * dxx * gM)  # subs.f90:169


def grad_mag(src, nx, ny, nz, dx, T):
    """weno (subs.f90:489-711) on every interior cell 1..n-1 of src (shape (nx+1, ny+1, nz+1)); returns gM."""
    I = slice(1, -1)
    c0 = src[I, I, I]
    # :657-662, the first-order branch
    a = (c0 - src[:-2, I, I]) / dx
    b = (src[2:, I, I] - c0) / dx
    c = (c0 - src[I, :-2, I]) / dx
    d = (src[I, 2:, I] - c0) / dx
    e = (c0 - src[I, I, :-2]) / dx
    f = (src[I, I, 2:] - c0) / dx
    # :506: i > 3 and i < nx-4, the same in j and k
    if nx - 4 > 4 and ny - 4 > 4 and nz - 4 > 4:
        bi, bj, bk = slice(4, nx - 4), slice(4, ny - 4), slice(4, nz - 4)

        def sh(s, m):
            return slice(s.start + m, s.stop + m)

        wa, wb = weno_axis([src[sh(bi, m), bj, bk] for m in range(-3, 4)], dx, False, T)
        wc, wd = weno_axis([src[bi, sh(bj, m), bk] for m in range(-3, 4)], dx, True, T)
        we, wf = weno_axis([src[bi, bj, sh(bk, m)] for m in range(-3, 4)], dx, False, T)
        box = (sh(bi, -1), sh(bj, -1), sh(bk, -1))
        for lo, hi in ((a, wa), (b, wb), (c, wc), (d, wd), (e, we), (f, wf)):
            lo[box] = hi
    return godunov(c0, a, b, c, d, e, f, T)


def sweep_jacobi(phi, phiS, nx, ny, nz, dx, h, T):
    """update_cell (subs.f90:747-750) on every interior cell, all reads from the old field; returns the new array."""
    I = slice(1, -1)
    gM = grad_mag(phi, nx, ny, nz, dx, T)
    sgn = phisign(phiS[I, I, I], dx, gM)
    k1 = sgn * (T(1.) - gM)
    out = phi.copy(order="F")
    out[I, I, I] = phi[I, I, I] + h * k1
    return out


def bc_closed(phi, nx, ny, nz, dx):
    """oracle bc_closed, in place: a wall point takes the interior value at the clamped index and adds dx
    m = min(nb, 1 + nh) times in sequence."""
    i, j, k = np.ogrid[0:nx + 1, 0:ny + 1, 0:nz + 1]
    nb = ((i == 0) | (i == nx)).astype(int) + ((j == 0) | (j == ny)) + ((k == 0) | (k == nz))
    nh = (i == nx).astype(int) + (j == ny) + (k == nz)
    m = np.minimum(nb, 1 + nh)
    v = phi[np.clip(i, 1, nx - 1), np.clip(j, 1, ny - 1), np.clip(k, 1, nz - 1)]
    for t in range(3):
        v = np.where(m > t, v + dx, v)
    phi[...] = np.where(nb > 0, v, phi)


def rms_change(phi, phiN, nx, ny, nz, T):
    """oracle rms_change: sequential float64 sum of the squared differences, i outermost, k innermost, over all points."""
    d = (phi - phiN).astype(np.float64)
    err = np.cumsum((d * d).ravel(order="C"))[-1]
    if T is np.float32:
        den = float(nx) * float(ny) * float(nz)
    else:
        den = float(np.int32(np.uint32((nx * ny * nz) & 0xFFFFFFFF)))
    return float(np.sqrt(err / den))


def reinit(phi0, nx, ny, nz, iter, dx, h, tol=0.0, dtype=np.float64):
    """lsf_oracle_reinit with the Jacobi ordering and the closed-form BC.  Returns (field of `dtype`, sweeps, rms trace)."""
    T = np.float32 if np.dtype(dtype) == np.float32 else np.float64
    phi = np.array(phi0, dtype=T, order="F", copy=True)
    assert phi.shape == (nx + 1, ny + 1, nz + 1)
    dx, h = T(dx), T(h)
    phiS = phi.copy(order="F")  # subs.f90:731
    phiN = phi.copy(order="F")
    trace = []
    with np.errstate(all="ignore"):
        for _ in range(iter + 1):  # subs.f90:735
            phi = sweep_jacobi(phi, phiS, nx, ny, nz, dx, h, T)
            bc_closed(phi, nx, ny, nz, dx)
            err = rms_change(phi, phiN, nx, ny, nz, T)
            trace.append(err)
            if err < tol:  # :915
                break
            phiN = phi.copy(order="F")
            if np.isnan(err):  # :926
                break
    assert phi.dtype == T
    return phi, len(trace), np.array(trace)


def distance(got, ref):
    """(max, RMS) of got - ref in units of eps32 * max|ref|, both taken in float64."""
    err = np.asarray(got, dtype=np.float64) - ref
    unit = EPS32 * float(np.abs(ref).max())
    return float(np.abs(err).max()) / unit, float(np.sqrt(np.mean(err * err))) / unit
