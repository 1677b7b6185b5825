"""Normal orientation's speed (GPU box only).  Inputs, each at k = 30 with the
project's own KNN30 normals:
  1. the full bunny (tests/golden/bunny.pcd, 35 947 points);
  2. C2's voxel representatives (uniform 10M cloud, vs = (4/N)^(1/3): 2.47M
     points);
  3. "blobs 2M": tools/dbscan_time.py's generator (4 Gaussian blobs sigma 0.05
     + 12.5 % clutter) at 2M points;
  4. the bunny voxel-downsampled at 0.005 (3017 points, the fixture's case E),
     beside the numpy restatement's wall time on the same input.  The
     restatement (tests/orient_oracle.py) is an unoptimised, dense Python
     transcription, not a baseline; it is quadratic in memory, which is why it
     is timed on this input and not on the full bunny.
Every input runs in a child process of its own under its own time limit
(--limit-*).  A child prints the stage it enters, so a run that does not finish
leaves its stage on record; nothing is retried and no later input is started
after one that ran out of time.
Per input: the whole call (neighbour lists included) by the host clock around
--reps calls after a warm-up, each ending in a device synchronise (also with the
tree and flip outputs); the neighbour lists alone; per stage the
library's timers (o3dx_set_kernel_timing) in a separate set of calls: EMST (grid +
Boruvka rounds), normal MST (rounds), propagation (root search + sign flips);
the Boruvka rounds of both trees; the propagation's launch count, which is 3
whatever the tree's depth (the parities come out of the union-find).
Usage: python tools/orient_time.py [--reps 5] [--out profiles/orient_normals_time.txt]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open3d-py-extension_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orient_normals_time.txt"))
ap.add_argument("--input", default=None, help="(child) one of bunny, c2, blobs, bunny3017")
ap.add_argument("--limit-bunny", type=int, default=120)
ap.add_argument("--limit-c2", type=int, default=300)
ap.add_argument("--limit-blobs", type=int, default=300)
ap.add_argument("--limit-bunny3017", type=int, default=120)
args = ap.parse_args()
K = 30
TIMERS = ("emst_grid", "emst_round", "nmst_round", "orient_flip", "orient_sort")


def stage(name):
    print(json.dumps({"stage": name}), flush=True)


def blobs(n, seed=1):
    """tools/dbscan_time.py's generator"""
    import torch

    g = torch.Generator(device="cpu").manual_seed(seed)
    centres = torch.tensor([[0.25, 0.25, 0.3], [0.75, 0.3, 0.6], [0.3, 0.75, 0.7], [0.7, 0.75, 0.25]])
    nb = n * 7 // 32
    parts = [c + 0.05 * torch.randn((nb, 3), generator=g) for c in centres]
    parts.append(torch.rand((n - 4 * nb, 3), generator=g))
    p = torch.cat(parts)
    return p[torch.randperm(n, generator=g)].float().contiguous()


def child(which):
    import numpy as np
    import torch

    from open3dpypro import _native as N, ops, synthetic as S
    from open3dpypro.pcd_io import read_pcd_arrays

    dev = torch.device("cuda:0")
    stage("input")
    if which in ("bunny", "bunny3017"):
        f = read_pcd_arrays(os.path.join(ROOT, "tests", "golden", "bunny.pcd"))
        x = torch.as_tensor(np.stack([f["x"], f["y"], f["z"]], 1).astype(np.float32), device=dev)
        tag = "bunny"
        if which == "bunny3017":
            x = ops.voxel_down_sample(x, 0.005)["rep_xyz"].contiguous()
            tag = "bunny voxel 0.005"
    elif which == "c2":
        n2 = 10_000_000
        x = ops.voxel_down_sample(S.uniform_cube(n2, seed=0, device=dev), S.voxel_size_for(n2))["rep_xyz"].contiguous()
        tag = "C2 voxel representatives"
    else:
        x = blobs(2_000_000).to(dev)
        tag = "blobs 2M"
    nrm = ops.estimate_normals(x, knn=K).contiguous()
    torch.cuda.synchronize()
    n = int(x.shape[0])
    out = {"input": tag, "n": n, "k": K}

    def timed(fn, reps):  # host clock around calls that end in a device synchronise
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / reps, r

    stage("knn lists")
    ops.knn_search(x, x, N.SEARCH_KNN, K)
    out["knn_lists_ms"] = round(timed(lambda: ops.knn_search(x, x, N.SEARCH_KNN, K), args.reps)[0], 3)
    stage("emst (warm-up)")
    t0 = time.perf_counter()
    ops.emst(x)
    torch.cuda.synchronize()
    out["emst_first_call_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    stage("orient (warm-up: EMST, normal MST, propagation)")
    t0 = time.perf_counter()
    ops.orient_normals_tangent_plane(x, nrm, K)
    torch.cuda.synchronize()
    out["first_call_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    stage("orient (timed calls)")
    ms, _ = timed(lambda: ops.orient_normals_tangent_plane(x, nrm, K), args.reps)
    out["call_ms"] = round(ms, 3)
    out["call_with_tree_and_flips_ms"] = round(
        timed(lambda: ops.orient_normals_tangent_plane(x, nrm, K, return_tree=True), args.reps)[0], 3)
    stage("orient (stage timers)")
    N.set_kernel_timing(True)
    N.reset_kernel_timing()
    _, res = timed(lambda: ops.orient_normals_tangent_plane(x, nrm, K, return_tree=True), args.reps)
    tm = {name: N.kernel_timing(name) for name in TIMERS}
    N.set_kernel_timing(False)
    out["emst_ms"] = round((tm["emst_grid"][0] + tm["emst_round"][0]) / args.reps, 3)
    out["normal_mst_ms"] = round(tm["nmst_round"][0] / args.reps, 3)
    out["propagation_ms"] = round(tm["orient_flip"][0] / args.reps, 3)
    out["tree_sort_ms"] = round(tm["orient_sort"][0] / args.reps, 3)
    out["emst_rounds"] = tm["emst_round"][1] // args.reps
    out["normal_mst_rounds"] = tm["nmst_round"][1] // args.reps
    out["propagation_launches"] = 3
    out["flipped"] = int(res[2].sum().item())
    if which == "bunny3017":
        import orient_oracle as OO

        stage("numpy restatement")
        p, q = x.cpu().numpy(), nrm.cpu().numpy()
        t0 = time.perf_counter()
        r = OO.orient(p, q, K)
        out["numpy_restatement_wall_ms (unoptimised Python, not a baseline)"] = round(
            (time.perf_counter() - t0) * 1e3, 1)
        out["equal_to_restatement"] = bool(np.array_equal(res[1].cpu().numpy(), r["tree"])
                                           and np.array_equal(res[2].cpu().numpy(), r["flip"]))
    print(json.dumps(out), flush=True)


def main():
    lines = []
    for which in ("bunny", "bunny3017", "c2", "blobs"):
        limit = getattr(args, "limit_" + which)
        cmd = [sys.executable, os.path.abspath(__file__), "--input", which, "--reps", str(args.reps)]
        last, result = "start", None
        t0 = time.perf_counter()
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
            rc, text = p.returncode, p.stdout
            err = p.stderr
        except subprocess.TimeoutExpired as e:
            rc, text = "timeout", (e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or ""))
            err = ""
        for ln in text.splitlines():
            try:
                d = json.loads(ln)
            except ValueError:
                continue
            if "stage" in d:
                last = d["stage"]
            else:
                result = ln
        if result is not None and rc == 0:
            lines.append(result)
        else:
            lines.append(json.dumps({"input": which, "finished": False, "exit": rc, "limit_s": limit,
                                     "stage": last, "wall_s": round(time.perf_counter() - t0, 1),
                                     "stderr_tail": err[-300:]}))
        print(lines[-1], flush=True)
        if rc != 0:  # out of time or failed: nothing more is started on the GPU
            break
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for ln in lines:
            f.write(ln + "\n")


if __name__ == "__main__":
    if args.input:
        child(args.input)
    else:
        main()
