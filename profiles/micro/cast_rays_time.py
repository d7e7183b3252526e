"""Time lsf_cast_rays on a 512 x 512 pinhole image of two spheres, beside lsf_sample_points on as many points: ms per call at 256^3
and 512^3 (profiles/cast_rays_time.txt).

    python3 profiles/micro/cast_rays_time.py [--repeats 5] [--out FILE]

Case: the two spheres of the benchmark's field (radius 0.5 at (-0.6, 0, 0) and (0.6, 0, 0) on N^3 points over [-1.5, 1.5]^3) as their
exact distance min(d1, d2) -- the smeared sign the benchmark sweeps is no distance and has no band of 8.1 dx -- device seam.  Rays:
512 x 512 from the eye (0.3, -4, 0.8) through the screen [-0.8, 0.8] x [-0.2, 0.8] (x, z) in the wall y = -1.5, in image order (x
fastest): both spheres in view, the nearer edge of one in front of the other, about a third of the rays hit.  Timed: castRays
linear and cubic with safety 0.9, smin 0.05, refine 24, max_steps 4096: without a mask with smax = 1 (the default: a step stays in
the cells the last sample saw) and smax = 8 (the field is a distance); with the mask |phi| < 8.1 dx, smax = 1 and skip = 4.  Beside
them samplePoints with iters = 3, same order, on 512 x 512 points: the end of every ray's march (the hit, or where a miss left the box).
Per configuration the samples per ray, info[6] / nrays, and the strides per ray, info[7] / nrays.
Each N is a child process of its own under its own time limit; the next one is not started if one fails.  Per figure: host clock
around one call that ends in a synchronise, after one warm-up call; median and spread over `repeats` calls.
A record, not a gate.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LIMIT = 240  # seconds per case
SIZES = (256, 512)
W = 512

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--case", default=None, help="N (internal: one child process per size)")
args = ap.parse_args()

if args.case is None:
    rows = []
    for n in SIZES:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", str(n), "--repeats", str(args.repeats)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LIMIT)
        if r.returncode != 0:
            sys.exit(f"case {n} ended with status {r.returncode}: nothing more is started")
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = {"what": f"lsf_cast_rays on a {W} x {W} pinhole image of two spheres (exact distance), linear and cubic, without a mask (smax 1 and 8) and "
                   "with the mask |phi| < 8.1 dx (skip 4), beside lsf_sample_points with iters = 3 on as many points, device seam: ms per call "
                   f"(host clock around a call; median of {args.repeats} calls after a warm-up)",
           "command": "python3 profiles/micro/cast_rays_time.py", "rows": rows}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0)

import torch  # noqa: E402

sys.path.insert(0, ROOT)
import levelsetfortran_amd as L  # noqa: E402

N = int(args.case)
n = N - 1
dx = 3.0 / n
LO = (-1.5, -1.5, -1.5)
ax = -1.5 + dx * torch.arange(N, dtype=torch.float64, device="cuda")
X, Y, Z = ax[None, None, :], ax[None, :, None], ax[:, None, None]  # i is the unit-stride axis
phi = None
for c in ((-0.6, 0.0, 0.0), (0.6, 0.0, 0.0)):
    d = torch.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - 0.5
    phi = d if phi is None else torch.minimum(phi, d)
    del d
phi = phi.reshape(-1).contiguous()
mask = (phi.abs() < 8.1 * dx).to(torch.int32)


def timed(fn):
    ms = []
    for it in range(args.repeats + 1):  # the first call is the warm-up: workspace, code objects
        torch.cuda.synchronize()
        t = time.perf_counter()
        rep = fn()
        torch.cuda.synchronize()
        if it:
            ms.append((time.perf_counter() - t) * 1e3)
    med = statistics.median(ms)
    return med, (max(ms) - min(ms)) / med, rep


def fortran(p):
    """(m, 3) in Fortran order: the transpose of a contiguous (3, m)"""
    return p.t().contiguous().t()


eye = torch.tensor((0.3, -4.0, 0.8), dtype=torch.float64, device="cuda")
sz, sx = torch.meshgrid(torch.linspace(-0.2, 0.8, W, dtype=torch.float64, device="cuda"),
                        torch.linspace(-0.8, 0.8, W, dtype=torch.float64, device="cuda"), indexing="ij")  # x fastest
screen = torch.stack([sx.reshape(-1), torch.full((W * W,), -1.5, dtype=torch.float64, device="cuda"), sz.reshape(-1)], dim=1)
org = fortran(eye.expand(W * W, 3).clone())
dirs = fortran(screen - eye)
nrays = W * W
base = dict(safety=0.9, smin=0.05, refine=24, max_steps=4096, want_hit=False, want_grad=True)
row = {"N": N, "device": torch.cuda.get_device_name(0), "rays": nrays, "list_cells": int(mask.sum())}
ends = None
for order in ("linear", "cubic"):
    for name, kw in (("smax1", dict(smax=1.0)), ("smax8", dict(smax=8.0)), ("mask_skip4", dict(smax=1.0, skip=4.0, mask=mask))):
        med, spread, rep = timed(lambda: L.castRays(phi, n, n, n, dx, LO, org, dirs, order=order, **base, **kw))
        key = f"{order}_{name}"
        row[f"{key}_ms"], row[f"{key}_spread"], row[f"{key}_info"] = med, spread, list(rep.info)
        row[f"{key}_samples_per_ray"], row[f"{key}_strides_per_ray"] = rep.info[6] / nrays, rep.info[7] / nrays
        assert rep.info[3] == 0 and rep.info[2] == 0
        if ends is None:  # the end of every march: the hit, or where the ray left the box
            u = dirs / torch.linalg.norm(dirs, dim=1, keepdim=True)
            t = torch.nan_to_num(rep.thit, nan=2.6)
            ends = fortran(org + t[:, None] * u)
    med, spread, rep = timed(lambda: L.samplePoints(phi, n, n, n, dx, LO, ends, order=order, iters=3, tol=1e-6))
    row[f"{order}_sample_iters3_ms"], row[f"{order}_sample_iters3_spread"], row[f"{order}_sample_iters3_info"] = med, spread, list(rep.info)
print(f"# {N}^3: linear {row['linear_smax1_ms']:.3f} / smax 8 {row['linear_smax8_ms']:.3f} / mask {row['linear_mask_skip4_ms']:.3f} ms, cubic "
      f"{row['cubic_smax1_ms']:.3f} / {row['cubic_smax8_ms']:.3f} / {row['cubic_mask_skip4_ms']:.3f} ms; samplePoints {row['linear_sample_iters3_ms']:.3f} / "
      f"{row['cubic_sample_iters3_ms']:.3f} ms", file=sys.stderr, flush=True)
print(json.dumps(row))
