"""ISS keypoints' speed (GPU box only), steady state.  Inputs:
  1. the bunny (35 947 points) at automatic radii and at (0.01, 0.008), the
     fixture's widest neighbourhoods (up to 390 points);
  2. a synthetic surface: 1M uniform samples of a box surface (float32) at
     automatic radii;
  3. the same kind of surface as a float64 scan (synthetic.las_scene, 1M) at
     automatic radii: the *_f64 entries.
Per input and per form of the sweep (O3DX_ISS_FORM=tile|lane, the same
passes): the model resolution, and the whole call by HIP events (mean of --reps
calls after a warm-up); the grid builds and the three passes by the library's
timers (o3dx_set_kernel_timing, a separate set of calls: kp_grid is the mean
over the builds of all three passes, kp_count the uncapped count at the
salient radius).  The outputs of the two forms are compared bit for bit.  The
bunny is also timed on the CPU restatement (tests/iss_oracle.py, one host
thread; skipped with --no-cpu).  The last line names the faster form per pass.
Usage: python tools/iss_keypoints_time.py [--reps 5] [--no-cpu]"""
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
from open3dpypro import _native as N, ops, synthetic as S  # noqa: E402
from open3dpypro.pcd_io import read_pcd_arrays  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--no-cpu", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda:0")
PASSES = ("kp_grid", "kp_count", "kp_saliency", "kp_nms")


def events(fn):
    fn()  # warm-up (workspace, code objects)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(args.reps):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, round(a.elapsed_time(b) / args.reps, 3)


def measure(tag, x, sr, nr):
    res = None
    if sr == 0.0:
        res, res_ms = events(lambda: ops.model_resolution(x))
        sr, nr = 6.0 * res, 4.0 * res
    results = {}
    rows = []
    for form in ("tile", "lane"):
        os.environ["O3DX_ISS_FORM"] = form
        out = {"input": tag, "n": int(x.shape[0]), "dtype": str(x.dtype).replace("torch.", ""), "form": form,
               "salient_radius": round(sr, 6), "non_max_radius": round(nr, 6)}
        if res is not None:
            out["resolution_ms"] = res_ms
        (idx, _, _), out["call_ms"] = events(lambda: ops.iss_keypoints(x, sr, nr))
        N.set_kernel_timing(True)
        N.reset_kernel_timing()
        for _ in range(args.reps):
            cnt = ops.radius_count(x, sr)
            s, c2 = ops.iss_saliency(x, sr)
            i2 = ops.iss_nms(x, s, nr)
        torch.cuda.synchronize()
        for name in PASSES:
            tot, k = N.kernel_timing(name)
            out[name + "_ms"] = round(tot / max(k, 1), 3)
        N.set_kernel_timing(False)
        out["keypoints"] = int(idx.numel())
        out["mean_neighbourhood"] = round(float(cnt.double().mean().item()), 2)
        out["max_neighbourhood"] = int(cnt.max().item())
        results[form] = (cnt.cpu(), s.cpu(), i2.cpu(), idx.cpu())
        rows.append(out)
    same = all(torch.equal(u, v) for u, v in zip(results["tile"], results["lane"]))
    for out in rows:
        out["forms_bit_identical"] = same
        print(json.dumps(out), flush=True)
    return rows, sr, nr


f = read_pcd_arrays(os.path.join(ROOT, "tests", "golden", "bunny.pcd"))
bunny = np.stack([f["x"], f["y"], f["z"]], 1).astype(np.float32)
xb = torch.as_tensor(bunny, device=dev)
allrows = []
rows, sr, nr = measure("bunny, automatic radii", xb, 0.0, 0.0)
allrows += rows
if not args.no_cpu:
    import iss_oracle as O

    t0 = time.perf_counter()
    r = O.iss(bunny, sr, nr)
    dt = time.perf_counter() - t0
    print(json.dumps({"input": "bunny, automatic radii", "cpu_restatement_ms": round(dt * 1e3, 1),
                      "keypoints": int(len(r["keypoints"]))}), flush=True)
allrows += measure("bunny, radii (0.01, 0.008)", xb, 0.01, 0.008)[0]
allrows += measure("box surface 1M", S.box_surface(1_000_000, seed=4, device=dev).contiguous(), 0.0, 0.0)[0]
allrows += measure("las_scene 1M float64", S.las_scene(1_000_000, seed=4, device=dev).contiguous(), 0.0, 0.0)[0]
won = {}
for name in ("kp_count", "kp_saliency", "kp_nms"):
    t = sum(r[name + "_ms"] for r in allrows if r["form"] == "tile")
    ln = sum(r[name + "_ms"] for r in allrows if r["form"] == "lane")
    won[name] = {"tile_ms_total": round(t, 3), "lane_ms_total": round(ln, 3), "faster": "tile" if t < ln else "lane"}
print(json.dumps({"faster_form_per_pass": won}), flush=True)
