"""Time redistanceBand beside reinitBand and one round of distanceFill on the same field and mask (profiles/redistance_band_time.txt).

    python3 profiles/micro/redistance_band_time.py [--repeats 5] [--out FILE]

Field: the two-sphere distance d of profiles/micro/extend_band_time.py (radii 0.5 and 0.35, the second one leaving through a wall) on
N^3 points of [-1.5, 1.5]^3, times g = 1 + 0.1 x + 0.05 sin 3z, made on the device; mask |d| < 8.1 dx; near = 2.5, iters = 8,
tol = 1e-9.  N = 256 and 512, device seam, each case a child process of its own under its own time limit; a case is not started if
the one before failed.  Host clock around calls that end in a synchronise, median of `repeats` calls after one warm-up, every call on a
fresh copy of the field.  redistanceBand is timed twice: to convergence, and with max_passes = 1 -- list build, foot launch, seed,
one pass and the finish -- so that the difference divided by the passes beyond the first is the cost of a pass and the rest is the
fixed part of a call.  The foot launch cannot be timed by itself through the interface; samplePoints on the list cells' own points
with the same mask, order, iters and tol does the same samples and projections in one launch (points in memory order instead of brick
order, and it writes val, grad, foot and status besides) and is timed as its stand-in.  Beside them: reinitBand with iter = 19
(20 sweeps, tol = 0, fast arithmetic) and distanceFill with band = 2.5 and max_rounds = 1.  A record, not a gate: there is no
threshold.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LIMITS = {256: 180, 512: 420}  # seconds per case
NEAR, WIDTH, ITERS, TOL = 2.5, 8.1, 8, 1e-9

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--case", type=int, choices=sorted(LIMITS), default=None)
args = ap.parse_args()

if args.case is None:
    rows = {}
    for N in sorted(LIMITS):
        cmd = [sys.executable, os.path.abspath(__file__), "--case", str(N), "--repeats", str(args.repeats)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LIMITS[N])
        if r.returncode != 0:
            sys.exit(f"case {N} ended with status {r.returncode}: nothing more is started")
        rows[str(N)] = json.loads(r.stdout.strip().splitlines()[-1])
    out = {"what": "two-sphere distance times 1 + 0.1 x + 0.05 sin 3z on N^3 points, mask |d| < 8.1 dx, near 2.5, device seam: redistanceBand, "
                   f"reinitBand (20 sweeps) and one round of distanceFill; host clock, ms per call (median of {args.repeats})",
           "command": "python3 profiles/micro/redistance_band_time.py", **rows}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0)

import torch  # noqa: E402

sys.path.insert(0, ROOT)
import levelsetfortran_amd as L  # noqa: E402
from levelsetfortran_amd import fields  # noqa: E402

N = args.case
n = N - 1
dx = 3.0 / n
ax = -1.5 + torch.arange(N, dtype=torch.float64, device="cuda") * dx
X, Y, Z = ax[None, None, :], ax[None, :, None], ax[:, None, None]  # (nz+1, ny+1, nx+1): i is the unit-stride axis


def sphere(cx, cy, cz, r):
    return torch.sqrt((X - cx) ** 2 + (Y - cy) ** 2 + (Z - cz) ** 2) - r


d = torch.minimum(sphere(-0.3, 0.2, 0.1, 0.5), sphere(1.3, 0.6, -0.2, 0.35)).contiguous()
phi0 = (d * (1.0 + 0.1 * X + 0.05 * torch.sin(3.0 * Z))).contiguous()
mask = (d.abs() < WIDTH * dx).to(torch.int32).contiguous()
del X, Y, Z
# the list cells as points of the grid with xLo = 0, (npts, 3) in Fortran order, for the stand-in of the foot launch
inner = torch.zeros_like(mask, dtype=torch.bool)
inner[1:-1, 1:-1, 1:-1] = mask[1:-1, 1:-1, 1:-1] == 1
kji = torch.nonzero(inner)
pts = (kji.flip(1).to(torch.float64) * dx).t().contiguous().t()
del inner, kji


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


def run(fn, fresh):
    work = fresh.clone()
    fn(work)  # warm-up: workspace, code objects
    ms = []
    for _ in range(args.repeats):
        work.copy_(fresh)
        t, rep = timed(lambda: fn(work))
        ms.append(t)
    return ms, rep


kw = dict(near=NEAR, iters=ITERS, tol=TOL)
t_all, rep = run(lambda a: L.redistanceBand(a, mask, n, n, n, dx, max_passes=64, **kw), phi0)
t_one, rep1 = run(lambda a: L.redistanceBand(a, mask, n, n, n, dx, max_passes=1, **kw), phi0)
t_foot, rep_s = run(lambda a: L.samplePoints(a, n, n, n, dx, (0.0, 0.0, 0.0), pts, order="cubic", mask=mask, iters=ITERS, tol=TOL), phi0)
t_reinit, rep_r = run(lambda a: L.reinitBand(a, mask, n, n, n, 19, dx, fields.reinit_step(dx), tol=0.0), phi0)
t_fill, rep_f = run(lambda a: L.distanceFill(a, n, n, n, dx, band=NEAR, max_rounds=1), d)
assert rep.converged and rep1.passes == 1 and rep1.cells == rep.cells == pts.shape[0] and rep_r.count == 20
all_ms, one_ms = statistics.median(t_all), statistics.median(t_one)
per_pass = (all_ms - one_ms) / max(rep.passes - 1, 1)
row = {"redistance_ms": all_ms, "redistance_ms_samples": t_all, "passes": rep.passes, "trace": rep.trace, "report": list(rep[3:]),
       "one_pass_ms": one_ms, "one_pass_ms_samples": t_one, "ms_per_pass": per_pass, "fixed_ms": one_ms - per_pass,
       "foot_stand_in_ms": statistics.median(t_foot), "foot_stand_in_ms_samples": t_foot,
       "reinit_band_20_sweeps_ms": statistics.median(t_reinit), "reinit_band_ms_samples": t_reinit,
       "distance_fill_one_round_ms": statistics.median(t_fill), "distance_fill_ms_samples": t_fill,
       "list_share_of_grid": rep.cells / float(N) ** 3, "device": torch.cuda.get_device_name(0), "grid": [N, N, N]}
print(f"# {N}^3: redistanceBand {all_ms:.3f} ms / {rep.passes} passes on {rep.cells} cells ({per_pass:.4f} ms per pass, {one_ms - per_pass:.3f} ms "
      f"fixed, foot stand-in {row['foot_stand_in_ms']:.3f}); reinitBand 20 sweeps {row['reinit_band_20_sweeps_ms']:.3f} ms; distanceFill one round "
      f"{row['distance_fill_one_round_ms']:.2f} ms", file=sys.stderr, flush=True)
print(json.dumps(row))
