"""Time lsf_reinit_band against the full-grid Jacobi reinit at 512^3 (profiles/reinit_band_512.json).

    python3 profiles/micro/reinit_band_time.py [--n 512] [--repeats 3] [--commit ID] [--box NAME] [--out FILE]

Field: the exact signed distance to two spheres (c = (-+0.6, 0, 0), R = 0.5) on [-1.5, 1.5]^3 in HBM, so that |phi| < w dx is a tube of
w cells on either side of the surface (fields.two_sphere_phi0 is the SMEARED SIGN of that distance: its |phi| < w dx is a fraction of a
cell wide).  h = fields.reinit_step(dx), device seam, tol = 0.  Masks: |phi| < w dx for w in {4.1, 8.1, 16, 32}, and every point.
Per mask and arithmetic: list length; per-sweep time = slope between a 50-sweep and a 250-sweep call (host clock around calls that
end in a synchronise), per-call overhead = the intercept; the same slope for reinit(order="jacobi") of the same arithmetic.  Band and
full grid alternate in ONE process, `repeats` times; spread = (max - min) / median of the repeats' slopes.  Prints one JSON line.
"""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import levelsetfortran_amd as L  # noqa: E402
from levelsetfortran_amd import fields  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=512)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--commit", default=None)
ap.add_argument("--box", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
N = args.n
n = N - 1
dev = torch.device("cuda", 0)
SHORT, LONG = 50, 250


def distance_field():
    dx = 3.0 / (N - 1)
    x = -1.5 + dx * torch.arange(N, dtype=torch.float64, device=dev)
    d = None
    for c in ((-0.6, 0.0, 0.0), (0.6, 0.0, 0.0)):
        r = ((x[:, None, None] - c[2]) ** 2 + (x[None, :, None] - c[1]) ** 2 + (x[None, None, :] - c[0]) ** 2).sqrt_().sub_(0.5)
        d = r if d is None else torch.minimum(d, r)
        del r
    return d.reshape(-1), dx


def timed(fn, phi0, work):
    work.copy_(phi0)
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn(work)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def fit(t_short, t_long):
    slope = (t_long - t_short) / (LONG - SHORT)
    return slope, t_short - SHORT * slope


phi0, dx = distance_field()
h = fields.reinit_step(dx)
work = torch.empty_like(phi0)
inner = torch.zeros((N, N, N), dtype=torch.bool, device=dev)
inner[1:n, 1:n, 1:n] = True
inner = inner.reshape(-1)
masks = [(f"{w}", (phi0.abs() < w * dx).to(torch.int32)) for w in (4.1, 8.1, 16, 32)] + [("all", torch.ones(phi0.numel(), dtype=torch.int32, device=dev))]
rows = []
for arith in ("fast", "strict"):
    def full(k):
        return lambda f: L.reinit(f, None, None, n, n, n, k - 1, dx, h, tol=0.0, order="jacobi", arith=arith)

    for name, m in masks:
        nL = int(((m == 1) & inner).sum())

        def band(k, m=m):
            return lambda f: L.reinitBand(f, m, n, n, n, k - 1, dx, h, tol=0.0, arith=arith)

        timed(band(SHORT), phi0, work), timed(full(SHORT), phi0, work)  # warm-up: workspace, code objects
        bs, fs, bi, fi = [], [], [], []
        for _ in range(args.repeats):  # band / full / band / full
            b50 = timed(band(SHORT), phi0, work)
            f50 = timed(full(SHORT), phi0, work)
            b250 = timed(band(LONG), phi0, work)
            f250 = timed(full(LONG), phi0, work)
            s, i = fit(b50, b250)
            bs.append(s), bi.append(i)
            s, i = fit(f50, f250)
            fs.append(s), fi.append(i)
        med = statistics.median
        row = {"arith": arith, "mask": name, "list_cells": nL, "list_fraction": nL / phi0.numel(),
               "band_ms_per_sweep": med(bs), "band_ms_per_sweep_samples": bs, "band_spread": (max(bs) - min(bs)) / med(bs),
               "band_call_overhead_ms": med(bi),
               "full_ms_per_sweep": med(fs), "full_ms_per_sweep_samples": fs, "full_spread": (max(fs) - min(fs)) / med(fs),
               "full_call_overhead_ms": med(fi),
               "band_ms_per_million_list_cells": med(bs) / (nL / 1e6), "full_over_band": med(fs) / med(bs)}
        rows.append(row)
        print(f"# {arith} w={name}: list {nL} ({100 * row['list_fraction']:.2f} %), band {row['band_ms_per_sweep']:.4f} ms/sweep "
              f"(+{row['band_call_overhead_ms']:.2f} ms/call, spread {100 * row['band_spread']:.1f} %), full {row['full_ms_per_sweep']:.4f} "
              f"(spread {100 * row['full_spread']:.1f} %), ratio {row['full_over_band']:.2f}", file=sys.stderr, flush=True)

# list fraction at which a band sweep costs what a full-grid sweep costs: least-squares line through the band's per-sweep times
cross = {}
for arith in ("fast", "strict"):
    rs = [r for r in rows if r["arith"] == arith]
    xs, ys = [r["list_cells"] for r in rs], [r["band_ms_per_sweep"] for r in rs]
    mx, my = sum(xs) / len(xs), sum(ys) / len(ys)
    b = sum((x - mx) * (y - my) for x, y in zip(xs, ys)) / sum((x - mx) ** 2 for x in xs)
    a = my - b * mx
    full_ms = statistics.median(r["full_ms_per_sweep"] for r in rs)
    cross[arith] = {"band_ms_per_sweep_fixed": a, "band_ms_per_million_list_cells": b * 1e6, "full_ms_per_sweep": full_ms,
                    "crossover_list_fraction": (full_ms - a) / b / phi0.numel()}

commit = args.commit
if commit is None:
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        commit = "unknown"
out = {"what": f"lsf_reinit_band against reinit(order='jacobi') at {N}^3, exact two-sphere distance field, device seam, tol = 0; per-sweep time = "
               f"slope between a {SHORT}-sweep and a {LONG}-sweep call, band / full alternating in one process, {args.repeats} repeats",
       "command": "python3 profiles/micro/reinit_band_time.py", "commit": commit, "box": args.box or socket.gethostname(),
       "device": torch.cuda.get_device_name(0), "grid": [N, N, N], "rows": rows, "crossover": cross}
line = json.dumps(out)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
