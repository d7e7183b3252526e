"""Time extendField per round and, beside it, distanceFill per round on the same field: the two have the same launch structure (8 x
(tiles_x + tiles_y + tiles_z - 2) dependent launches of 32 x 8 x 8-point tiles per round), the extension loads two fields per tile
and keeps two LDS images (profiles/extend_field_time.txt).

    python3 profiles/micro/extend_field_time.py [--repeats 3] [--out FILE]

Field: the distance to two spheres (radii 0.5 and 0.35, the second one leaving through a wall) on N^3 points of [-1.5, 1.5]^3, made
on the device; frozen band 3.5 cells; q = 1 + 0.5 x - 0.3 y + 0.2 z^2 on the band.  N = 256 and 512, device seam, each case a child
process of its own under its own time limit; a case is not started if the one before failed.  Host clock around calls that end in a
synchronise, median of `repeats` calls after one warm-up, divided by the rounds the call ran (check, init and count passes included).
A record, not a gate: there is no threshold.  Prints one JSON line.
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
BAND = 3.5

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=3)
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
    out = {"what": "two-sphere distance on N^3 points, frozen band 3.5 cells, device seam: extendField and distanceFill on the same field; "
                   f"host clock, ms per call (median of {args.repeats}) and ms per round",
           "command": "python3 profiles/micro/extend_field_time.py", **rows}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0)

import torch  # noqa: E402

sys.path.insert(0, ROOT)
import levelsetfortran_amd as L  # noqa: E402

N = args.case
n = N - 1
dx = 3.0 / n
ax = -1.5 + torch.arange(N, dtype=torch.float64, device="cuda") * dx
X, Y, Z = ax[None, None, :], ax[None, :, None], ax[:, None, None]  # (nz+1, ny+1, nx+1): i is the unit-stride axis


def sphere(cx, cy, cz, r):
    return torch.sqrt((X - cx) ** 2 + (Y - cy) ** 2 + (Z - cz) ** 2) - r


phi = torch.minimum(sphere(-0.3, 0.2, 0.1, 0.5), sphere(1.3, 0.6, -0.2, 0.35)).contiguous()
q0 = (1.0 + 0.5 * X - 0.3 * Y + 0.2 * Z * Z).expand_as(phi).contiguous()
del X, Y, Z


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


t_ext, rep_e = run(lambda a: L.extendField(a, phi, n, n, n, dx, band=BAND), q0)
t_df, rep_d = run(lambda a: L.distanceFill(a, n, n, n, dx, band=BAND), phi)
assert rep_e.frozen_points == rep_d.frozen_points
tiles = -(-N // 32) + 2 * -(-N // 8) - 2
row = {"extend_ms": statistics.median(t_ext), "extend_ms_samples": t_ext, "extend_rounds": rep_e.rounds, "extend_changed": rep_e.changed,
       "extend_ms_per_round": statistics.median(t_ext) / rep_e.rounds,
       "fill_ms": statistics.median(t_df), "fill_ms_samples": t_df, "fill_rounds": rep_d.rounds, "fill_changed": rep_d.changed,
       "fill_ms_per_round": statistics.median(t_df) / rep_d.rounds,
       "extend_converged": rep_e.converged, "fill_converged": rep_d.converged, "unreached": rep_e.unreached,
       "frozen_points": rep_e.frozen_points, "launches_per_round": 8 * tiles, "device": torch.cuda.get_device_name(0), "grid": [N, N, N]}
print(f"# {N}^3: extendField {row['extend_ms']:.2f} ms / {rep_e.rounds} rounds = {row['extend_ms_per_round']:.2f} ms per round; "
      f"distanceFill {row['fill_ms']:.2f} ms / {rep_d.rounds} rounds = {row['fill_ms_per_round']:.2f} ms per round", file=sys.stderr, flush=True)
print(json.dumps(row))
