"""The grid, the fields and the ray sets of tests/test_gpu_cast_rays.py, shared with tests/test_cast_rays_cpu.py, which asserts on the
statement alone that the sets are what they claim to be.

Grid: nx, ny, nz = 12, 9, 7 cells (13 x 10 x 8 points): three different strides, cubic cells on every axis; dx and xLo are binary
fractions.  phi is a sphere of 1.25 cells radius plus a smooth perturbation -- the level set lies in the cells whose cubic stencil is
interior, so that it can be hit under a mask -- and, beside it along x, a second sphere of 0.75 cells for occlusion; q another
smooth field; the mask phi < 4.1 dx (the bodies and a band around them) with a hole (0) over the back of the first sphere, two more
(7, -1) near the walls and 1s on the walls, which no list holds.  smax = 0.5 and max_steps = 32 let the longest rays run out of steps.
Rays (nrays in 1, 63, 65, 256, 2037: one lane, a ragged wave, a wave and a lane, a block, eight blocks the last ragged), shuffled
once: a pinhole fan from outside the box looking along +x, random rays from around the box aimed into it, axis-parallel rays in all
six directions, rays from inside the bodies, and the special rays (zero, NaN, +-inf, 1e300, on and off the walls)."""
import functools

import numpy as np

import cast_ref as C

N = (12, 9, 7)
SHAPE = tuple(n + 1 for n in N)
DX, LO = 0.125, (-0.75, 0.25, 1.0)
C1, R1 = (-0.25, 0.8125, 1.4375), 0.15625
C2, R2 = (0.375, 0.8125, 1.4375), 0.09375
NRAYS = [1, 63, 65, 256, 2000 + 37]
PAR = dict(iso=0.02, tmin=0.0, tmax=2.75, safety=0.9, smin=0.05, smax=0.5, skip=0.75, refine=20, max_steps=32)
INSTANCES = [(o, hm, hq) for o in (C.LINEAR, C.CUBIC) for hm in (False, True) for hq in (False, True)]


@functools.lru_cache(maxsize=None)
def fields():
    """(phi, mask, q), shared and read-only"""
    ax = [LO[A] + np.arange(SHAPE[A]) * DX for A in range(3)]
    x, y, z = np.meshgrid(*ax, indexing="ij")
    s1 = np.sqrt((x - C1[0]) ** 2 + (y - C1[1]) ** 2 + (z - C1[2]) ** 2) - R1 + 0.02 * np.sin(3.0 * x) * np.cos(2.0 * y + z)
    s2 = np.sqrt((x - C2[0]) ** 2 + (y - C2[1]) ** 2 + (z - C2[2]) ** 2) - R2
    phi = np.asfortranarray(np.minimum(s1, s2))
    q = np.asfortranarray(1.25 + 0.5 * x - np.sin(2.0 * y) * (0.75 + z))
    mask = np.asfortranarray((phi < 4.1 * DX).astype(np.int32))
    mask[0, :, :] = mask[-1, :, :] = mask[:, 0, :] = mask[:, -1, :] = mask[:, :, 0] = mask[:, :, -1] = 1  # 1s on the walls: in no list
    mask[6, 4, 4], mask[11, 4, 3], mask[1, 8, 6] = 0, 7, -1  # a hole between the spheres, over the back of the first one; two near the walls
    for a in (phi, mask, q):
        a.setflags(write=False)
    return phi, mask, q


def special_rays():
    nan, inf = float("nan"), float("inf")
    mid = [LO[A] + 0.5 * N[A] * DX for A in range(3)]
    hi = [LO[A] + N[A] * DX for A in range(3)]
    rays = [
        ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), (mid, (0.0, 0.0, 0.0)), ((nan, mid[1], mid[2]), (1.0, 0.0, 0.0)), (mid, (nan, 1.0, 0.0)),
        ((inf, mid[1], mid[2]), (-1.0, 0.0, 0.0)), (mid, (0.0, -inf, 0.0)), (mid, (1e300, 0.0, 0.0)), ((1e300, mid[1], mid[2]), (-1.0, 0.0, 0.0)),
        ((-1e300, 1e300, mid[2]), (1.0, -1.0, 0.0)), (mid, (1e-300, 0.0, 0.0)), (mid, (0.0, 0.0, -1e-200)),
        # along x on the walls and one step beyond them
        ((-2.0, LO[1], mid[2]), (1.0, 0.0, 0.0)), ((-2.0, hi[1], mid[2]), (1.0, 0.0, 0.0)), ((-2.0, float(np.nextafter(hi[1], 9.0)), mid[2]), (1.0, 0.0, 0.0)),
        ((-2.0, mid[1], float(np.nextafter(LO[2], 0.0))), (1.0, 0.0, 0.0)), ((-2.0, mid[1], LO[2]), (3.0, 0.0, 0.0)),
        # from a wall inwards and outwards, from a corner along the diagonal, along an edge
        ((hi[0], mid[1], mid[2]), (-1.0, 0.0, 0.0)), ((hi[0], mid[1], mid[2]), (1.0, 0.0, 0.0)), ((LO[0], mid[1], mid[2]), (1.0, 0.0, 0.0)),
        (LO, (1.0, 1.0, 1.0)), (hi, (-1.0, -0.75, -0.5)), (LO, (1.0, 0.0, 0.0)), ((-2.0, -1.0, mid[2]), (1.25, 1.25, 0.0)),
        # -0.0 in the origin and the direction
        ((-0.0, mid[1], mid[2]), (-0.0, 1.0, -0.0)), ((-0.0, mid[1], 3.0), (0.0, -0.0, -1.0)),
    ]
    return np.array([r[0] for r in rays], dtype=np.float64), np.array([r[1] for r in rays], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def rays(nrays):
    """(org, dir): (nrays, 3) each, in Fortran order, read-only; the first nrays of one shuffled set of 2037"""
    rng = np.random.default_rng(2037)
    lo, n = np.asarray(LO), np.asarray(N)
    mid = lo + 0.5 * n * DX
    so, sd = special_rays()
    # a pinhole fan: 26 x 24 pixels of a screen in the plane x = 0
    py, pz = np.meshgrid(np.linspace(0.55, 1.05, 26), np.linspace(1.2, 1.7, 24), indexing="ij")
    eye = np.array([-2.0, 0.85, 1.4])
    fan_d = np.stack([np.zeros(py.size), py.ravel(), pz.ravel()], axis=1) - eye
    fan_o = np.broadcast_to(eye, fan_d.shape)
    # random rays from a shell around the box aimed at points near the bodies
    m = 900
    v = rng.standard_normal((m, 3))
    ro = mid + (1.2 + 0.8 * rng.random(m))[:, None] * v / np.linalg.norm(v, axis=1)[:, None]
    aim = np.where(rng.random(m)[:, None] < 0.7, np.asarray(C1), np.asarray(C2)) + 0.16 * (rng.random((m, 3)) - 0.5)
    rd = (aim - ro) * (0.25 + 3.0 * rng.random(m))[:, None]
    # axis-parallel rays, all six directions, through points near the bodies
    k = 340
    axis = rng.integers(0, 3, k)
    sign = rng.choice([-1.0, 1.0], k)
    ad = np.zeros((k, 3))
    ad[np.arange(k), axis] = sign * (0.5 + rng.random(k))
    through = np.where(rng.random(k)[:, None] < 0.75, np.asarray(C1), np.asarray(C2)) + 0.2 * (rng.random((k, 3)) - 0.5)
    ao = through.copy()
    ao[np.arange(k), axis] -= sign * 1.5
    # rays that begin inside the bodies
    b = 2037 - len(so) - len(fan_o) - m - k
    w = rng.standard_normal((b, 3))
    bo = np.asarray(C1) + 0.5 * R1 * rng.random(b)[:, None] * w / np.linalg.norm(w, axis=1)[:, None]
    bd = rng.standard_normal((b, 3))
    org = np.concatenate([so, fan_o, ro, ao, bo])
    dir_ = np.concatenate([sd, fan_d, rd, ad, bd])
    assert len(org) == 2037 and b > 100
    perm = rng.permutation(2037)
    org, dir_ = np.asfortranarray(org[perm][:nrays]), np.asfortranarray(dir_[perm][:nrays])
    for a in (org, dir_):
        a.setflags(write=False)
    return org, dir_


@functools.lru_cache(maxsize=None)
def want(order, hasmask, hasq, nrays):
    phi, mask, q = fields()
    org, dir_ = rays(nrays)
    return C.cast_rays(phi, DX, LO, org, dir_, order=order, mask=mask if hasmask else None, q=q if hasq else None, **PAR)
