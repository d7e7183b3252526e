"""The fields and masks of the lsf_label_band tests (tests/test_label_band_cpu.py, tests/test_gpu_label_band.py): the smallest on
which each piece can go wrong (a chunk is 256 list entries, MB_CH in csrc/lsf_minmax_band.hpp; a brick is 8 x 8 x 4 points).

  onecell      (10,10,10): one list cell
  small        (10,10,10): a sphere, |phi| < 2.1 dx: 246 cells, one ragged chunk; the inner shell is one component and the outer one
  two          (40,33,27): min of two sphere distances, every interior point listed: 2 INSIDE, 1 OUTSIDE; the last chunk is ragged
  hollow       (25,25,25): a spherical shell body, every interior point listed: 1 INSIDE, 2 OUTSIDE (cavity and exterior)
  hollow_band  the same field under the mask |phi| < 1.6 dx: every component has cells at the edge of the list
  snake_end    (17,17,9): a serpentine channel one cell wide, phi = -1 on it and +1 elsewhere, every interior point listed.  It runs
               through the eight rows j = 1, 3, ... 15 of each of the planes k = 1, 3, 5, 7 and the single cells that join them:
               511 cells that form ONE path, so the graph diameter of the component is its cell count.  The smallest index, (1,1,1),
               is one end of the path.
  snake_mid    the same planes joined at the other corners: (1,1,1) lies 126 cells from one end and 384 from the other
  checker      (12,11,10): phi = +-1 with the parity of i+j+k, every interior point listed: every cell is its own component
  values       (12,11,10): the mask of test_gpu_curvature_band.py's `values` case: 0, 7, -1, and 1s on wall points
  iso          (12,11,10), iso = 0.25: a sphere distance with points planted at exactly 0.25 (d = +0.0: OUTSIDE) and one ulp to either
               side, inside and outside the sphere, every interior point listed
  negzero      (12,11,10), iso = 0: -0.0 and 0.0 planted (d = -0.0 and +0.0: both OUTSIDE).  phi - 0.25 is never -0.0 in
               round-to-nearest -- a difference of two doubles is zero only when they are equal, and is then +0.0 -- so the signed
               zero of the contract is exercised where it can occur, with iso = 0.
"""
import functools

import numpy as np

import advect_ref as R

CENTRE, RADIUS = (0.1, 0.0, -0.1), 0.6
CASES = ["onecell", "small", "two", "hollow", "hollow_band", "snake_end", "snake_mid", "checker", "values", "iso", "negzero"]
NPTS = {"onecell": (10, 10, 10), "small": (10, 10, 10), "two": (40, 33, 27), "hollow": (25, 25, 25), "hollow_band": (25, 25, 25),
        "snake_end": (17, 17, 9), "snake_mid": (17, 17, 9), "checker": (12, 11, 10), "values": (12, 11, 10), "iso": (12, 11, 10),
        "negzero": (12, 11, 10)}
ISO = {"iso": 0.25}
ALL_ONES = ["two", "hollow", "snake_end", "snake_mid", "checker", "iso", "negzero"]
SNAKE_CELLS = 511


def snake_path(variant):
    """the cells of the channel in path order"""
    def plane(k, up):
        rows = range(1, 16, 2) if up else range(15, 0, -2)
        out, forward = [], True
        for n, j in enumerate(rows):
            out += [(i, j, k) for i in (range(1, 16) if forward else range(15, 0, -1))]
            if n < 7:
                out.append((15 if forward else 1, j + (1 if up else -1), k))
            forward = not forward
        return out  # begins and ends at i = 1

    if variant == "end":  # (1,1,1) first; joined at (1,15,2), (1,1,4), (1,15,6)
        path, up = [], True
        for k in (1, 3, 5, 7):
            path += plane(k, up)
            if k < 7:
                path.append((1, 15 if up else 1, k + 1))
            up = not up
        return path
    # plane 1 backwards, ending at (1,1,1); then (1,1,2) and upwards, joined at (1,15,4), (1,1,6)
    path, up = plane(1, True)[::-1], True
    for k in (3, 5, 7):
        path.append((1, 1 if up else 15, k - 1))
        path += plane(k, up)
        up = not up
    return path


@functools.lru_cache(maxsize=None)
def geometry(case):
    """(phi, mask, npts, iso) of a case; shared and read-only"""
    npts = NPTS[case]
    phi, dx = R.sphere_distance(npts, CENTRE, RADIUS)
    mask = np.ones(npts, np.int32)
    if case == "onecell":
        mask[...] = 0
        mask[4, 4, 4] = 1
    elif case == "small":
        mask = (np.abs(phi) < 2.1 * dx).astype(np.int32)
    elif case == "two":
        a, _ = R.sphere_distance(npts, (-0.6, 0.0, -0.2), 0.4)
        b, _ = R.sphere_distance(npts, (0.6, 0.1, -0.1), 0.45)
        phi = np.minimum(a, b)
    elif case in ("hollow", "hollow_band"):
        r, _ = R.sphere_distance(npts, (0.0, 0.0, 0.0), 0.0)
        phi = np.abs(r - 0.7) - 0.25
        if case == "hollow_band":
            mask = (np.abs(phi) < 1.6 * dx).astype(np.int32)
    elif case in ("snake_end", "snake_mid"):
        phi = np.ones(npts)
        for c in snake_path(case[6:]):
            phi[c] = -1.0
    elif case == "checker":
        i, j, k = np.meshgrid(*(np.arange(n) for n in npts), indexing="ij")
        phi = np.where((i + j + k) % 2 == 0, -1.0, 1.0)
    elif case == "values":
        band = np.abs(phi) < 1.3 * dx
        mask = np.where(band, 1, 0).astype(np.int32)
        mask[~band & (phi > 3.5 * dx)] = 7  # not 1: not in the list
        mask[~band & (phi < 0)] = -1
        for a in range(3):  # 1s on all six walls: ignored
            sl = [slice(None)] * 3
            for side in (0, -1):
                sl[a] = side
                mask[tuple(sl)] = 1
    elif case == "iso":
        phi = phi.copy(order="F")
        inner = np.argwhere(phi[1:-1, 1:-1, 1:-1] < 0.25 - dx) + 1  # points deep on the INSIDE of phi = 0.25
        for n, v in zip((0, len(inner) // 2, len(inner) - 1), (0.25, np.nextafter(0.25, 1.0), np.nextafter(0.25, 0.0))):
            phi[tuple(inner[n])] = v
        outer = np.argwhere(phi[1:-1, 1:-1, 1:-1] > 0.25 + dx) + 1
        phi[tuple(outer[len(outer) // 3])] = 0.25
        phi[tuple(outer[len(outer) // 2])] = np.nextafter(0.25, 0.0)
    elif case == "negzero":
        phi = phi.copy(order="F")
        inner = np.argwhere(phi[1:-1, 1:-1, 1:-1] < -dx) + 1
        phi[tuple(inner[0])], phi[tuple(inner[len(inner) // 2])], phi[tuple(inner[-1])] = -0.0, 0.0, -0.0
    phi, mask = np.asfortranarray(phi, dtype=np.float64), np.asfortranarray(mask)
    phi.setflags(write=False), mask.setflags(write=False)
    return phi, mask, npts, ISO.get(case, 0.0)


def prefill(npts):
    """label as the caller hands it in: -7 and 2^31 - 1 alternating"""
    a = np.full(int(np.prod(npts)), -7, np.int32)
    a[1::2] = 0x7fffffff
    return np.asfortranarray(a.reshape(npts, order="F"))


def two_sphere_chain(npts=(33, 33, 33)):
    """the merge case: two spheres with a gap of a few cells and the constant normal speed that closes it.
    Returns (phi0, mask0, speed, dx, dt, steps): mask0 is |phi0| < 6.1 dx, evolveBand's defaults do the rest."""
    a, dx = R.sphere_distance(npts, (-0.62, 0.0, 0.0), 0.45)
    b, _ = R.sphere_distance(npts, (0.62, 0.0, 0.0), 0.45)
    phi = np.asfortranarray(np.minimum(a, b))
    mask = np.asfortranarray((np.abs(phi) < 6.1 * dx).astype(np.int32))
    speed = np.ones(npts, order="F")
    return phi, mask, speed, dx, 0.5 * dx, 7
