"""DBSCAN's speed (GPU box only), steady state.  Inputs:
  1. C2's voxel representatives (uniform 10M cloud, vs = (4/N)^(1/3): 2.47M
     points) at eps = 2 vs, min_samples 10;
  2. the fixture's blobs generator (4 Gaussian blobs sigma 0.05 + 12.5 %
     clutter) at 2M points, min_samples 6, eps = 0.04 scaled by (3200 / n)^(1/3)
     so the neighbourhoods keep the 3200-point case's size (at eps 0.04 a blob's
     centre would hold ~6e4 neighbours per point);
  3. 200k uniform points at eps 0.012, min_samples 5: the input sklearn is
     timed on (host CPU, all of it; skipped with --no-sklearn).
Per input: the whole call by HIP events (mean of --reps calls after a
warm-up), the grid build and the four passes by the library's timers
(o3dx_set_kernel_timing: events around each pass, in a separate set of calls),
and the mean neighbourhood size |N(i)| (self included) over 1000 sampled
points, since the time scales with it.
Usage: python tools/dbscan_time.py [--reps 5] [--no-sklearn]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open3d-py-extension_amd"))
from open3dpypro import _native as N, ops, synthetic as S  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--no-sklearn", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda:0")
PASSES = ("dbscan_grid", "dbscan_core", "dbscan_union", "dbscan_label", "dbscan_border")


def blobs(n, seed=1):
    g = torch.Generator(device="cpu").manual_seed(seed)
    centres = torch.tensor([[0.25, 0.25, 0.3], [0.75, 0.3, 0.6], [0.3, 0.75, 0.7], [0.7, 0.75, 0.25]])
    nb = n * 7 // 32
    parts = [c + 0.05 * torch.randn((nb, 3), generator=g) for c in centres]
    parts.append(torch.rand((n - 4 * nb, 3), generator=g))
    p = torch.cat(parts)
    return p[torch.randperm(n, generator=g)].float().contiguous()


def mean_neighbourhood(x, eps, samples=1000):
    idx = torch.linspace(0, x.shape[0] - 1, samples, device=x.device).long()
    xd = x.double()
    tot = 0
    for s in range(0, samples, 20):
        q = xd[idx[s:s + 20]]
        d2 = ((q[:, None, :] - xd[None, :, :]) ** 2).sum(-1)
        tot += int((d2 <= eps * eps).sum().item())
    return tot / samples


def measure(tag, x, eps, ms):
    out = {"input": tag, "n": int(x.shape[0]), "eps": round(float(eps), 6), "min_samples": ms}
    labels, k = ops.dbscan(x, eps, ms)  # warm-up (workspace, code objects)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.reps):
        labels, k = ops.dbscan(x, eps, ms)
    b.record()
    torch.cuda.synchronize()
    out["call_ms"] = round(a.elapsed_time(b) / args.reps, 3)
    N.set_kernel_timing(True)
    N.reset_kernel_timing()
    for _ in range(args.reps):
        ops.dbscan(x, eps, ms)
    torch.cuda.synchronize()
    for name in PASSES:
        tot, cnt = N.kernel_timing(name)
        out[name + "_ms"] = round(tot / max(cnt, 1), 3)
    N.set_kernel_timing(False)
    out["clusters"] = k
    out["noise"] = int((labels < 0).sum().item())
    out["mean_neighbourhood"] = round(mean_neighbourhood(x, eps), 2)
    print(json.dumps(out), flush=True)
    return labels


n2 = 10_000_000
vs = S.voxel_size_for(n2)
reps = ops.voxel_down_sample(S.uniform_cube(n2, seed=0, device=dev), vs)["rep_xyz"].contiguous()
measure("C2 voxel representatives", reps, 2 * vs, 10)
del reps
nb = 2_000_000
measure("blobs 2M", blobs(nb).to(dev), 0.04 * (3200 / nb) ** (1 / 3), 6)
small = S.uniform_cube(200_000, seed=2, device=dev)
lab = measure("uniform 200k", small, 0.012, 5)
if not args.no_sklearn:
    from sklearn.cluster import DBSCAN

    p = small.cpu().numpy().astype(np.float64)
    t0 = time.perf_counter()
    m = DBSCAN(eps=0.012, min_samples=5).fit(p)
    dt = time.perf_counter() - t0
    print(json.dumps({"input": "uniform 200k", "sklearn_cpu_ms": round(dt * 1e3, 1), "host_cpus": os.cpu_count(),
                      "labels_equal": bool(np.array_equal(m.labels_, lab.cpu().numpy()))}), flush=True)
