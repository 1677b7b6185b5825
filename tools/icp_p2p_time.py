"""Point-to-point against point-to-plane ICP on the device loop (GPU box only),
same build, same clouds: C3's ICP input (box-surface target and an
independent sample of it moved by T_gt, 10M points each, max_corr 0.02), one
target built with normals (it serves both estimations), the source sorted
once, 30 iterations from T = I with no convergence stop.
Per estimation: the whole loop by HIP events (each of --reps calls after a
warm-up, and their mean: the spread is what a difference has to exceed), the
per-step kernel time and the loop's own events by the library's timers
(o3dx_set_kernel_timing, in a separate set of calls), iterations per second,
and the share of queries the skip proof still searches (the debug search
counters, one more call).  The estimations converge at different rates, so
the skip proof leaves them different amounts of searching; two further legs
compare the steps like for like: the same loops with the skip proof off
(O3DX_ICP_SKIP=0: every step searches every query) and one accumulate step
(the plain step kernel) at the same T, the identity and the planted motion.
Usage: python tools/icp_p2p_time.py [--n 10000000] [--iters 30] [--reps 5]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open3d-py-extension_amd"))
from open3dpypro import _native as N, ops, synthetic as S  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10_000_000)
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
dev = torch.device("cuda:0")

tgt = S.box_surface(args.n, seed=1, device=dev)
src = S.apply_transform(S.box_surface(args.n, seed=2, device=dev), S.rigid_transform())
target = ops.ICPTarget(tgt, ops.estimate_normals(tgt, knn=30), 0.02)
src4 = ops.spatial_sort(src)
gt = np.linalg.inv(S.rigid_transform())


def measure(estimation, with_scaling, skip=True):
    os.environ["O3DX_ICP_SKIP"] = "1" if skip else "0"  # read by the library at every call
    kw = dict(max_iteration=args.iters, relative_fitness=0.0, relative_rmse=0.0, estimation=estimation,
              with_scaling=with_scaling)
    out = {"leg": "loop", "estimation": estimation, "with_scaling": with_scaling, "skip_proof": skip, "n": args.n,
           "iterations": args.iters}
    res = target.register(src4, **kw)  # warm-up (workspace, code objects)
    torch.cuda.synchronize()
    calls = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = target.register(src4, **kw)
        b.record()
        torch.cuda.synchronize()
        calls.append(a.elapsed_time(b))
    out["loop_ms_calls"] = [round(c, 3) for c in calls]
    out["loop_ms"] = round(float(np.mean(calls)), 3)
    out["iters_per_s"] = round(args.iters / (float(np.mean(calls)) * 1e-3), 1)
    N.set_kernel_timing(True)
    N.reset_kernel_timing()
    for _ in range(args.reps):
        target.register(src4, **kw)
    torch.cuda.synchronize()
    m_ms, m_n = N.kernel_timing("icp_match")
    l_ms, l_n = N.kernel_timing("icp_loop")
    N.set_kernel_timing(False)
    out["step_kernel_ms"] = round(m_ms / max(m_n, 1), 4)
    out["step_launches_per_call"] = m_n // max(args.reps, 1)
    out["loop_events_ms"] = round(l_ms / max(l_n, 1), 3)
    N.search_stats(True)
    target.register(src4, **kw)
    out["searched_share"] = round(N.search_stats()["queries"] / ((args.iters + 1) * args.n), 4)
    N.search_stats(False)
    out["fitness"] = round(res["fitness"], 6)
    out["inlier_rmse"] = float(res["inlier_rmse"])
    out["T_err_vs_gt_inverse"] = float(np.abs(res["transformation"] - gt).max())
    print(json.dumps(out), flush=True)


def measure_step(estimation, T, tag):
    """one accumulate (the plain step kernel + the digit collect) at a fixed T"""
    target.accumulate(src4, T, estimation=estimation)  # warm-up
    N.set_kernel_timing(True)
    N.reset_kernel_timing()
    for _ in range(args.reps):
        sums, _ = target.accumulate(src4, T, estimation=estimation)
    torch.cuda.synchronize()
    m_ms, m_n = N.kernel_timing("icp_match")
    N.set_kernel_timing(False)
    print(json.dumps({"leg": "accumulate", "estimation": estimation, "T": tag, "n": args.n,
                      "step_kernel_ms": round(m_ms / max(m_n, 1), 4), "launches": m_n,
                      "matched": int(sums[28])}), flush=True)


measure("point_to_plane", False)
measure("point_to_point", False)
measure("point_to_point", True)
measure("point_to_plane", False)  # once more: the drift over the run
measure("point_to_plane", False, skip=False)
measure("point_to_point", False, skip=False)
measure("point_to_plane", False, skip=False)
for tag, T in (("identity", np.eye(4)), ("planted motion", gt)):
    for est in ("point_to_plane", "point_to_point", "point_to_plane", "point_to_point"):
        measure_step(est, T, tag)
