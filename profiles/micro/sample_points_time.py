"""Time lsf_sample_points at the nodes of extractSurface, in cell order and shuffled, beside lsf_curvature_band on the same field: ms
per call at 256^3 and 512^3 (profiles/sample_points_time.txt).

    python3 profiles/micro/sample_points_time.py [--repeats 5] [--out FILE]

Case: that of profiles/micro/curvature_band_time.py -- the exact distance to a sphere of radius 0.5 at (-0.15, -0.1, 0.05) on N^3
points over [-1.5, 1.5]^3, device seam.  Points: (a) the nodes extractSurface returns, which arrive in cell order, (b) the same nodes in
a shuffled order (a fixed permutation).  Timed: samplePoints linear and cubic, value and gradient, without a projection and with
iters = 3 (the nodes lie on the surface, so the loop ends at its first test; a second set, the nodes pushed 1.5 dx along the outward
normal, makes it move); cubic with q = kappa and the mask |phi| < 8.1 dx; lsf_curvature_band (kappa only) on that mask beside them.
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
    out = {"what": "lsf_sample_points at the nodes of extractSurface (cell order and shuffled) beside lsf_curvature_band on the mask |phi| < 8.1 dx of "
                   f"the same field, device seam: ms per call (host clock around a call; median of {args.repeats} calls after a warm-up)",
           "command": "python3 profiles/micro/sample_points_time.py", "rows": rows}
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
C = (-0.15, -0.1, 0.05)
ax = -1.5 + dx * torch.arange(N, dtype=torch.float64, device="cuda")
X, Y, Z = ax[None, None, :], ax[None, :, None], ax[:, None, None]  # i is the unit-stride axis
phi = (torch.sqrt((X - C[0]) ** 2 + (Y - C[1]) ** 2 + (Z - C[2]) ** 2) - 0.5).reshape(-1).contiguous()
mask = (phi.abs() < 8.1 * dx).to(torch.int32)
kappa = torch.full_like(phi, float("nan"))


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
    """(npts, 3) in Fortran order: the transpose of a contiguous (3, npts)"""
    return p.t().contiguous().t()


row = {"N": N, "device": torch.cuda.get_device_name(0)}
med, spread, rep = timed(lambda: L.curvatureBand(phi, mask, n, n, n, dx, kappa))
row.update(curvature_ms=med, curvature_spread=spread, list_cells=rep.cells)
nodes = L.extractSurface(phi, n, n, n, dx, LO)[0]
npts = int(nodes.shape[0])
row.update(nodes=npts)
perm = torch.randperm(npts, generator=torch.Generator().manual_seed(1)).cuda()
centre = torch.tensor(C, dtype=torch.float64, device="cuda")
unit = (nodes - centre) / torch.linalg.norm(nodes - centre, dim=1, keepdim=True)
sets = {"nodes": nodes, "shuffled": fortran(nodes[perm]), "pushed": fortran(nodes + 1.5 * dx * unit), "pushed_shuffled": fortran((nodes + 1.5 * dx * unit)[perm])}
for name, pts in sets.items():
    for order in ("linear", "cubic"):
        if name.startswith("pushed"):
            med, spread, rep = timed(lambda: L.samplePoints(phi, n, n, n, dx, LO, pts, order=order, iters=3, tol=1e-6))
            row[f"{name}_{order}_iters3_ms"], row[f"{name}_{order}_iters3_spread"], row[f"{name}_{order}_iters3_info"] = med, spread, list(rep.info)
            continue
        med, spread, rep = timed(lambda: L.samplePoints(phi, n, n, n, dx, LO, pts, order=order))
        row[f"{name}_{order}_ms"], row[f"{name}_{order}_spread"] = med, spread
        assert rep.info[0] == npts
        med, spread, rep = timed(lambda: L.samplePoints(phi, n, n, n, dx, LO, pts, order=order, iters=3, tol=1e-6))
        row[f"{name}_{order}_iters3_ms"], row[f"{name}_{order}_iters3_spread"], row[f"{name}_{order}_iters3_info"] = med, spread, list(rep.info)
    med, spread, rep = timed(lambda: L.samplePoints(phi, n, n, n, dx, LO, pts, order="cubic", mask=mask, q=kappa))
    row[f"{name}_cubic_q_mask_ms"], row[f"{name}_cubic_q_mask_spread"], row[f"{name}_cubic_q_mask_info"] = med, spread, list(rep.info)
    if not name.startswith("pushed"):
        row[f"{name}_mean_kappa"] = float(rep.qval.mean())
print(f"# {N}^3: {npts} nodes; linear {row['nodes_linear_ms']:.3f} / shuffled {row['shuffled_linear_ms']:.3f} ms, cubic {row['nodes_cubic_ms']:.3f} / "
      f"{row['shuffled_cubic_ms']:.3f} ms; curvature {row['curvature_ms']:.3f} ms", file=sys.stderr, flush=True)
print(json.dumps(row))
