"""Global registration's speed (GPU box only), steady state.  Inputs:
  1. the bunny pair of the tests (tests/globalreg_cases.py: 2203 source and
     3017 target points, FPFH Hybrid(0.025, 64), distance 0.0075);
  2. two 100k-point synthetic.box_surface clouds (seeds 0 and 1), the source
     moved by synthetic.rigid_transform(30.0); normals KNN 30, FPFH
     Hybrid(0.03, 64), distance 0.015.
Per input, HIP-event means of --reps calls after a warm-up: FPFH of the target
(the whole call: neighbour search + both passes) and its two passes by the
library's timers (fpfh_spfh, fpfh_gather), the matcher (one direction, by its
timer, and the mutual correspondences call), one RANSAC round of 4096
hypotheses (host Umeyama + checkers by the wall clock, the corr_count sweep by
its timer) and the whole registration_ransac_based_on_feature_matching call
(wall clock: it is host-paced).
Usage: python tools/global_registration_time.py [--reps 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open3d-py-extension_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
from open3dpypro import (CorrespondenceCheckerBasedOnDistance, CorrespondenceCheckerBasedOnEdgeLength,  # noqa: E402
                         KDTreeSearchParamHybrid, KDTreeSearchParamKNN, PointCloud, RANSACConvergenceCriteria)
from open3dpypro import _native as N, ops, synthetic as S  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
dev = torch.device("cuda:0")


def events(fn):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) / args.reps, 3)


def timers(fn, names):
    N.set_kernel_timing(True)
    N.reset_kernel_timing()
    for _ in range(args.reps):
        fn()
    torch.cuda.synchronize()
    out = {}
    for name in names:
        tot, cnt = N.kernel_timing(name)
        out[name + "_ms"] = round(tot / max(cnt, 1), 4)
    N.set_kernel_timing(False)
    return out


def measure(tag, src, tgt, fpfh_param, max_d, seed):
    out = {"input": tag, "ns": src.size(), "nt": tgt.size(), "fpfh": repr(fpfh_param), "max_distance": max_d}
    mode, knn, radius = 2, fpfh_param.max_nn, fpfh_param.radius
    x, nr = tgt._dev_points(), tgt._normals
    out["fpfh_call_ms"] = events(lambda: ops.fpfh(x, nr, mode, knn, radius))
    out.update(timers(lambda: ops.fpfh(x, nr, mode, knn, radius), ("fpfh_spfh", "fpfh_gather")))
    fs = src.compute_fpfh_feature(fpfh_param)
    ft = tgt.compute_fpfh_feature(fpfh_param)
    a, b = fs.device_rows(), ft.device_rows()
    out.update(timers(lambda: ops.feature_match(a, b), ("feature_match",)))
    out["correspondences_mutual_ms"] = events(lambda: ops.correspondences_from_features(a, b, True))
    corres = ops.correspondences_from_features(a, b, True)
    C = int(corres.shape[0])
    out["correspondences"] = C
    # one round of 4096 hypotheses
    smp = ops.ransac_samples(C, 3, 4096, seed)
    ch = corres.cpu().numpy()
    ps = src._dev_points().cpu().numpy().astype(np.float64)[ch[:, 0]]
    qt = tgt._dev_points().cpu().numpy().astype(np.float64)[ch[:, 1]]
    coords = np.stack([ps[smp], qt[smp]], axis=2)
    t0 = time.perf_counter()
    for _ in range(args.reps):
        T = ops.umeyama_from_samples(coords)
        ok = ops.corr_check(coords, T, 0.9, max_d)
    out["round_host_ms"] = round((time.perf_counter() - t0) * 1e3 / args.reps, 3)
    out["round_survivors"] = int(ok.sum())
    sp, tp = src._dev_points(), tgt._dev_points()
    out["corr_count_4096_call_ms"] = events(lambda: ops.corr_count(sp, tp, corres, T, max_d))
    out.update(timers(lambda: ops.corr_count(sp, tp, corres, T, max_d), ("corr_count",)))
    checkers = [CorrespondenceCheckerBasedOnEdgeLength(0.9), CorrespondenceCheckerBasedOnDistance(max_d)]

    def whole():
        return src.registration_ransac_based_on_feature_matching(
            tgt, fs, ft, True, max_d, checkers=checkers, criteria=RANSACConvergenceCriteria(100000, 0.999), seed=seed)

    r = whole()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.reps):
        r = whole()
    torch.cuda.synchronize()
    out["ransac_call_ms"] = round((time.perf_counter() - t0) * 1e3 / args.reps, 3)
    out["fitness"] = round(float(r.fitness), 4)
    print(json.dumps(out), flush=True)
    return r


import globalreg_cases as GC  # noqa: E402
from open3dpypro.pcd_io import read_pcd_arrays  # noqa: E402

fl = read_pcd_arrays(os.path.join(ROOT, "tests", "golden", "bunny.pcd"))
s_np, t_np, T_true = GC.bunny_pair(np.stack([fl["x"], fl["y"], fl["z"]], 1).astype(np.float32))
src, tgt = PointCloud(s_np), PointCloud(t_np)
src.estimate_normals(param=KDTreeSearchParamHybrid(*GC.BUNNY_NORMALS_SRC))
tgt.estimate_normals(param=KDTreeSearchParamHybrid(*GC.BUNNY_NORMALS_TGT))
r = measure("bunny pair", src, tgt, KDTreeSearchParamHybrid(*GC.BUNNY_FPFH), GC.BUNNY_MAX_DIST, GC.BUNNY_SEED)
print(json.dumps({"input": "bunny pair", "pose_error_deg_and_length": GC.pose_error(r.transformation, T_true)}), flush=True)

n = 100_000
tgt = PointCloud(S.box_surface(n, seed=0, device=dev))
src = PointCloud(S.apply_transform(S.box_surface(n, seed=1, device=dev), S.rigid_transform(30.0)))
src.estimate_normals(param=KDTreeSearchParamKNN(30))
tgt.estimate_normals(param=KDTreeSearchParamKNN(30))
measure("box surface 100k", src, tgt, KDTreeSearchParamHybrid(0.03, 64), 0.015, 7)
