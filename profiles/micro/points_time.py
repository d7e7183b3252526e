"""Time lsf_advect_points and lsf_correct_field on the markers of seedParticles, beside lsf_sample_points on the same points and one
step of lsf_advect_field_band on the same mask: ms per call at 256^3 and 512^3 (profiles/points_time.txt).

    python3 profiles/micro/points_time.py [--repeats 5] [--out FILE]

Case: the exact distance to a sphere of radius 0.5 at (-0.15, -0.1, 0.05) on N^3 points over [-1.5, 1.5]^3, the mask |phi| < 8.1 dx,
a smooth velocity with |u|, |v|, |w| <= 1, dt = 0.4 dx, device seam.  Markers: seedParticles(per_cell=16), on the host, in the order it
returns them (cell after cell).  Timed: advectPoints, one RK3 step, linear and cubic, with and without the mask; correctField with and
without the mask on phi - 0.3 dx, which makes about 1 % of the markers escape (phi is restored before every call, outside the clock);
samplePoints(iters=0) on the same points, linear and cubic; advectFieldBand, one RK3 step on the mask.
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
LIMIT = 400  # seconds per case
SIZES = (256, 512)

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
    out = {"what": "lsf_advect_points (one RK3 step) and lsf_correct_field on the markers of seedParticles(per_cell=16), beside lsf_sample_points on "
                   "the same points and one step of lsf_advect_field_band on the mask |phi| < 8.1 dx, device seam: ms per call (host clock around a "
                   f"call; median of {args.repeats} calls after a warm-up)",
           "command": "python3 profiles/micro/points_time.py", "rows": rows}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, ROOT)
import levelsetfortran_amd as L  # noqa: E402

N = int(args.case)
n = N - 1
dx = 3.0 / n
LO = (-1.5, -1.5, -1.5)
C = (-0.15, -0.1, 0.05)
ax = -1.5 + dx * torch.arange(N, dtype=torch.float64, device="cuda")
X, Y, Z = ax[None, None, :], ax[None, :, None], ax[:, None, None]  # i is the unit-stride axis
phi = (torch.sqrt((X - C[0]) ** 2 + (Y - C[1]) ** 2 + (Z - C[2]) ** 2) - 0.5).reshape(-1).contiguous()
mask = (phi.abs() < 8.1 * dx).to(torch.int32)
full = lambda t: (t + 0.0 * (X + Y + Z)).reshape(-1).contiguous()
vel = (full(torch.sin(1.7 * Y + 0.4) * torch.cos(0.9 * Z)), full(torch.cos(1.3 * X - 0.2) * torch.sin(1.1 * Z + 0.5)), full(torch.sin(0.8 * X + 1.9 * Y)))
dt = 0.4 * dx


def timed(fn, prep=None):
    ms = []
    for it in range(args.repeats + 1):  # the first call is the warm-up: workspace, code objects
        if prep:
            prep()
        torch.cuda.synchronize()
        t = time.perf_counter()
        rep = fn()
        torch.cuda.synchronize()
        if it:
            ms.append((time.perf_counter() - t) * 1e3)
    med = statistics.median(ms)
    return med, (max(ms) - min(ms)) / med, rep


row = {"N": N, "device": torch.cuda.get_device_name(0)}
t0 = time.perf_counter()
host_phi = phi.cpu().numpy().reshape((N, N, N), order="F")
hp, hr = L.seedParticles(host_phi, n, n, n, dx, LO, per_cell=16)
row.update(markers=int(len(hr)), seed_s=time.perf_counter() - t0)
del host_phi
pts = torch.from_numpy(np.ascontiguousarray(hp.T)).cuda().t()
rad = torch.from_numpy(hr).cuda()
npts = int(len(hr))

for order in ("linear", "cubic"):
    med, spread, rep = timed(lambda: L.samplePoints(phi, n, n, n, dx, LO, pts, order=order, want_grad=False))
    row[f"sample_{order}_ms"], row[f"sample_{order}_spread"] = med, spread
    for m, name in ((None, "nomask"), (mask, "mask")):
        med, spread, rep = timed(lambda: L.advectPoints(pts, n, n, n, dx, LO, dt, 1, velocity=vel, mask=m, order=order, scheme="rk3"))
        row[f"advect_{order}_{name}_ms"], row[f"advect_{order}_{name}_spread"], row[f"advect_{order}_{name}_info"] = med, spread, list(rep.info)
    med, spread, rep = timed(lambda: L.advectPoints(pts, n, n, n, dx, LO, dt, 1, velocity=vel, speed=vel[0], phi=phi, mask=mask, order=order))
    row[f"advect_{order}_both_mask_ms"], row[f"advect_{order}_both_mask_spread"] = med, spread

shifted = phi - 0.3 * dx
work = shifted.clone()
for m, name in ((None, "nomask"), (mask, "mask")):
    med, spread, rep = timed(lambda: L.correctField(work, n, n, n, dx, LO, pts, rad, mask=m, slack=1.0), prep=lambda: work.copy_(shifted))
    row[f"correct_{name}_ms"], row[f"correct_{name}_spread"], row[f"correct_{name}_info"] = med, spread, list(rep.info)
    row[f"correct_{name}_change_dx"] = rep.change / dx
del shifted

band = phi.clone()
med, spread, rep = timed(lambda: L.advectFieldBand(band, mask, n, n, n, dx, dt, 1, velocity=vel), prep=lambda: band.copy_(phi))
row.update(advect_band_ms=med, advect_band_spread=spread, list_cells=int(rep.cells))
print(f"# {N}^3: {npts} markers; advectPoints cubic {row['advect_cubic_nomask_ms']:.3f} / masked {row['advect_cubic_mask_ms']:.3f} ms; correctField "
      f"{row['correct_nomask_ms']:.3f} / masked {row['correct_mask_ms']:.3f} ms; samplePoints cubic {row['sample_cubic_ms']:.3f} ms; "
      f"advectFieldBand {row['advect_band_ms']:.3f} ms", file=sys.stderr, flush=True)
print(json.dumps(row))
