"""Time lsf_reseed_points (call plus get) beside the host seedParticles on the same field, the copy home that call needs included, and
beside one lsf_correct_field: ms per call at 256^3 and 512^3 (profiles/reseed_time.txt).

    python3 profiles/micro/reseed_time.py [--repeats 5] [--out FILE]

Case: that of profiles/micro/points_time.py -- the exact distance to a sphere of radius 0.5 at (-0.15, -0.1, 0.05) on N^3 points over
[-1.5, 1.5]^3, the mask |phi| < 8.1 dx, a smooth velocity with |u|, |v|, |w| <= 1, dt = 0.4 dx, device seam.  Timed, with and without
the mask: reseedParticles from scratch (npts = 0; per_cell 16, band 3, cubic, iters 4, tol 1e-3), and a top-up of those markers after
they took 16 RK3 steps in the velocity (advectPoints, outside the clock); the host seedParticles(per_cell=16) with phi.cpu() inside the
clock; one correctField on the moved markers (phi restored before every call, outside the clock).
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
LIMIT = 420  # seconds per case
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
    out = {"what": "lsf_reseed_points + lsf_reseed_get (per_cell 16, band 3, cubic, iters 4, tol 1e-3) from scratch and as a top-up after 16 steps, "
                   "beside the host seedParticles(per_cell=16) with the copy of phi to the host, and one lsf_correct_field on the moved markers; "
                   f"sphere and mask |phi| < 8.1 dx of points_time.py, device seam: ms per call (host clock around a call; median of {args.repeats} "
                   "calls after a warm-up)",
           "command": "python3 profiles/micro/reseed_time.py", "rows": rows}
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
KW = dict(per_cell=16, rmin=0.1, rmax=0.5, band=3.0, order="cubic", iters=4, tol=1e-3)


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


def host_seed():
    host_phi = phi.cpu().numpy().reshape((N, N, N), order="F")  # the copy home that the host call needs
    return L.seedParticles(host_phi, n, n, n, dx, LO, per_cell=16)


ms, (hp, hr) = [], (None, None)
for it in range(2):  # seconds each: one warm-up, one figure
    torch.cuda.synchronize()
    t = time.perf_counter()
    hp, hr = host_seed()
    ms.append((time.perf_counter() - t) * 1e3)
row.update(host_seed_ms=ms[-1], host_seed_markers=int(len(hr)))
del hp, hr

for m, name in ((None, "nomask"), (mask, "mask")):
    med, spread, rep = timed(lambda: L.reseedParticles(phi, n, n, n, dx, LO, mask=m, seed=1, **KW))
    row[f"scratch_{name}_ms"], row[f"scratch_{name}_spread"], row[f"scratch_{name}_info"] = med, spread, list(rep.info)
    pts, rad = rep.pts, rep.rad
    for s in range(16):  # outside the clock
        pts = L.advectPoints(pts, n, n, n, dx, LO, dt, 1, velocity=vel, mask=m, order="cubic", scheme="rk3").pts
    med, spread, rep = timed(lambda: L.reseedParticles(phi, n, n, n, dx, LO, pts, rad, mask=m, seed=17, **KW))
    row[f"topup_{name}_ms"], row[f"topup_{name}_spread"], row[f"topup_{name}_info"] = med, spread, list(rep.info)
    row[f"topup_{name}_markers_in"] = int(rad.shape[0])
    work = phi.clone()
    med, spread, rep = timed(lambda: L.correctField(work, n, n, n, dx, LO, pts, rad, mask=m, slack=1.0), prep=lambda: work.copy_(phi))
    row[f"correct_{name}_ms"], row[f"correct_{name}_spread"], row[f"correct_{name}_info"] = med, spread, list(rep.info)
    del work, pts, rad
print(f"# {N}^3: host seedParticles with the copy home {row['host_seed_ms']:.0f} ms ({row['host_seed_markers']} markers); reseed from scratch "
      f"{row['scratch_nomask_ms']:.3f} / masked {row['scratch_mask_ms']:.3f} ms; top-up {row['topup_nomask_ms']:.3f} / masked "
      f"{row['topup_mask_ms']:.3f} ms; correctField {row['correct_nomask_ms']:.3f} / masked {row['correct_mask_ms']:.3f} ms", file=sys.stderr, flush=True)
print(json.dumps(row))
