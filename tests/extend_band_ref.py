"""Serial restatement of lsf_extend_field_band (include/lsf.h): a quantity q carried off the frozen cells of a cell list constant
along the normals of phi, by Jacobi passes of lsf_extend_field's visit over the list.

    LIST     the interior points (1..n-1 on each axis) with mask == 1 (advect_band_ref.list_of)
    FROZEN   the list cells with known == 1, or, without `known`, those with |phi| < band * dx
    pass     every non-frozen list cell is visited with q as it was at the start of the pass; an axis whose chosen neighbour (the
             one with the smaller |phi|, the lower index on a tie) is not in the list is not used -- the other neighbour is not tried

Two forms of the same loops:
  extend_band_loops   one cell at a time, double-buffered -- the contract read aloud;
  extend_band         numpy over the whole list.  |phi| never changes, so the neighbour each axis takes and its weight are fixed
                      for the call.
Both evaluate the visit exactly as the contract writes it (numpy fuses nothing; / is IEEE), so they agree bit for bit, and the GPU
tests compare with `extend_band`.  q off the list is never read: both forms work on a copy of q in which every point off the list
has been REPLACED BY A POISON VALUE first and put back at the end, so a result that equals the library's proves that neither reads
it there.

Layout: q, phi, mask, known are (nx+1, ny+1, nz+1).  The arguments are left alone.  Unknown is NaN.
"""
from __future__ import annotations

import functools
from typing import List, NamedTuple

import numpy as np

import advect_ref as R
import extend_ref as E
from advect_band_ref import list_of

POISON = -1.2345e300  # what the statement sees off the list instead of the caller's q


class ExtendBandResult(NamedTuple):
    field: np.ndarray
    passes: int
    trace: List[int]
    cells: int
    frozen: int
    reached: int
    unreached: int

    @property
    def converged(self):
        return bool(self.trace and self.trace[-1] == 0)

    @property
    def info(self):
        return [self.cells, self.frozen, self.reached, self.unreached]


def frozen_of(phi, lst, dx, band=None, known=None):
    """FROZEN as a boolean array.  With `known` the band is ignored, and so is `known` off the list."""
    if known is not None:
        return lst & (np.asarray(known) == 1)
    far = np.float64(band) * np.float64(dx)  # computed once
    with np.errstate(invalid="ignore"):
        return lst & (np.abs(phi) < far)


def check(q, phi, mask, dx, band=None, known=None):
    """(list cells, frozen cells, frozen cells with a non-finite q, list cells that see a non-finite phi at themselves or at one of
    their six neighbours): what the library counts before it writes."""
    phi = np.asarray(phi, dtype=np.float64)
    lst = list_of(mask)
    frozen = frozen_of(phi, lst, dx, band, known)
    bad = ~np.isfinite(phi)
    sees = bad.copy()
    for a in range(3):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[a], hi[a] = slice(None, -1), slice(1, None)
        sees[tuple(hi)] |= bad[tuple(lo)]
        sees[tuple(lo)] |= bad[tuple(hi)]
    return int(lst.sum()), int(frozen.sum()), int((frozen & ~np.isfinite(q)).sum()), int((lst & sees).sum())


def _start(q, phi, mask, dx, band, known):
    phi = np.asarray(phi, dtype=np.float64)
    lst = list_of(mask)
    frozen = frozen_of(phi, lst, dx, band, known)
    if not lst.any() or not frozen.any():
        raise ValueError("an empty list, or no frozen cell")
    Q = np.where(lst, np.where(frozen, np.asarray(q, dtype=np.float64), np.nan), POISON)
    return lst, frozen, np.abs(phi), Q


def _finish(q, lst, frozen, Q, trace):
    out = np.array(q, dtype=np.float64, copy=True, order="K")
    out[lst] = Q[lst]
    nan = np.isnan(out)
    return ExtendBandResult(out, len(trace), trace, int(lst.sum()), int(frozen.sum()), int((lst & ~frozen & ~nan).sum()),
                            int((lst & ~frozen & nan).sum()))


UNIT = ((1, 0, 0), (0, 1, 0), (0, 0, 1))


def extend_band_loops(q, phi, mask, dx, band=None, known=None, max_passes=256):
    lst, frozen, F, Q = _start(q, phi, mask, dx, band, known)
    cells = [tuple(c) for c in np.argwhere(lst & ~frozen)]
    trace = []
    while len(trace) < max_passes:
        old = Q.copy()  # all reads of a pass come before its writes
        changed = 0
        for p in cells:
            s, t = [], []
            for e in UNIT:
                lo = tuple(c - d for c, d in zip(p, e))
                hi = tuple(c + d for c, d in zip(p, e))
                n = hi if F[hi] < F[lo] else lo
                w = F[p] - F[n]
                if w > 0 and lst[n] and not np.isnan(old[n]):
                    s.append(w)
                    t.append(w * old[n])
                else:
                    s.append(np.float64(0.0))
                    t.append(np.float64(0.0))
            den = (s[0] + s[1]) + s[2]
            if den == 0:
                continue
            new = ((t[0] + t[1]) + t[2]) / den
            if not (new == old[p]):
                Q[p] = new
                changed += 1
        trace.append(changed)
        if changed == 0:
            break
    return _finish(q, lst, frozen, Q, trace)


def extend_band(q, phi, mask, dx, band=None, known=None, max_passes=256):
    lst, frozen, F, Q = _start(q, phi, mask, dx, band, known)
    at = np.argwhere(lst & ~frozen)
    own = tuple(at.T)
    # the plan: per axis the chosen neighbour and its weight, 0.0 where the axis can never be used
    nb, w = [], []
    for a in range(3):
        lo, hi = at.copy(), at.copy()
        lo[:, a] -= 1
        hi[:, a] += 1
        lo, hi = tuple(lo.T), tuple(hi.T)
        take_hi = F[hi] < F[lo]  # a tie takes the lower index
        n = tuple(np.where(take_hi, h, l) for h, l in zip(hi, lo))
        wa = F[own] - F[n]
        nb.append(n)
        w.append(np.where((wa > 0) & lst[n], wa, 0.0))
    trace = []
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        while len(trace) < max_passes:
            s, t = [], []
            for a in range(3):
                qn = Q[nb[a]]
                used = (w[a] > 0) & ~np.isnan(qn)
                s.append(np.where(used, w[a], 0.0))
                t.append(np.where(used, w[a] * qn, 0.0))
            den = (s[0] + s[1]) + s[2]
            new = ((t[0] + t[1]) + t[2]) / den
            store = (den != 0) & ~(new == Q[own])
            Q[tuple(c[store] for c in own)] = new[store]
            trace.append(int(store.sum()))
            if trace[-1] == 0:
                break
    return _finish(q, lst, frozen, Q, trace)


# ------------------------------------------------------------------------------------------------ the inputs the tests share
CENTRE, RADIUS = (0.1, 0.0, -0.1), 0.6  # the sphere of the other band tests
# case -> (points, width of the mask in cells or None for every point, frozen band in cells)
CASES = {"small": ((10, 10, 10), 2.1, 1.1), "general": ((40, 33, 27), 4.1, 1.5), "wide": ((40, 33, 27), 8.1, 1.5),
         "interior": ((25, 25, 25), None, 1.5), "onecell": ((10, 10, 10), None, 1.1), "values": ((12, 11, 10), 1.3, 0.8),
         "onesided": ((40, 33, 27), 4.1, None), "stop8": ((40, 33, 27), 2.6, 1.5), "stop9": ((40, 33, 27), 3.1, 1.5)}
FORMS = ("band", "known")


def prefill(npts, which=0):
    """a field as the caller hands it in: NaN and -7 alternating"""
    a = np.full(int(np.prod(npts)), np.nan)
    a[which::2] = -7.0
    return np.asfortranarray(a.reshape(npts, order="F"))


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(q, phi, mask, known, dx, band) of a named case, all read-only and Fortran-ordered.  phi is the distance to the sphere; q is
    extend_ref.quantity on the frozen cells and NaN / -7 alternating on every other point, list cells included: what a non-frozen
    cell holds on entry is ignored and nothing off the list is read.  `known` marks the frozen cells of the band form -- in
    "onesided" only those with phi > 0, and there is no band form -- and carries 1s on every point off the list, which are ignored.
      onecell   the list is one frozen cell and its x neighbour further from the surface
      values    a mask carrying 0, 7, -1, and 1s on wall points"""
    npts, width, band = CASES[case]
    phi, dx = R.sphere_distance(npts, CENTRE, RADIUS)
    if case == "onecell":
        f = np.abs(phi)
        a = next(tuple(p) for p in np.argwhere(f < band * dx)
                 if 1 <= p[0] < npts[0] - 2 and all(1 <= p[x] < npts[x] - 1 for x in (1, 2)) and f[p[0] + 1, p[1], p[2]] >= band * dx
                 and f[tuple(p)] <= f[p[0] + 2, p[1], p[2]])
        mask = np.zeros(npts, np.int32)
        mask[a] = mask[a[0] + 1, a[1], a[2]] = 1
    elif case == "values":
        near = np.abs(phi) < width * dx
        mask = np.where(near, 1, 0).astype(np.int32)
        mask[~near & (phi > 3.5 * dx)] = 7  # not 1: not in the list
        mask[~near & (phi < 0)] = -1
        for x in range(3):  # 1s on all six walls: ignored
            sl = [slice(None)] * 3
            for side in (0, -1):
                sl[x] = side
                mask[tuple(sl)] = 1
    elif width is None:
        mask = np.ones(npts, np.int32)
    else:
        mask = (np.abs(phi) < width * dx).astype(np.int32)
    mask = np.asfortranarray(mask)
    lst = list_of(mask)
    frozen = lst & (np.abs(phi) < 1.5 * dx) & (phi > 0) if case == "onesided" else frozen_of(phi, lst, dx, band)
    known = np.asfortranarray(np.where(lst, frozen, True).astype(np.int32))
    q = prefill(npts)
    q[frozen] = E.quantity(npts, dx)[frozen]
    for a in (q, phi, mask, known):
        a.setflags(write=False)
    return q, phi, mask, known, dx, band


@functools.lru_cache(maxsize=None)
def want(case, form, cap=256):
    q, phi, mask, known, dx, band = inputs(case)
    r = extend_band(q, phi, mask, dx, band=band if form == "band" else None, known=known if form == "known" else None, max_passes=cap)
    r.field.setflags(write=False)
    return r
