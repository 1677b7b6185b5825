"""LAS I/O speed (GPU box only).  10M point-format-3 records (34 bytes):
  1. o3dx_las_unpack (all outputs) and o3dx_las_pack (float64 points, colours,
     intensity, labels) on records already on the device: a host clock around
     synchronised calls, the median of --reps calls after a warm-up, and the
     bytes each call moves (records + arrays) over that time;
  2. the whole PointCloud.read_las(rgb, intensity, labels) of a 10M-point file
     in the page cache, beside the same file through the host numpy path
     (las_io.decode_host + PointCloud(...)), and read_las's parts timed alone:
     the file read (np.fromfile), the host-to-device copy of the records
     (pageable memory), the decode call with its flag read;
  3. the whole save_las of that cloud.
Usage: python tools/las_io_time.py [--n 10000000] [--reps 11] [--dir /tmp]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open3d-py-extension_amd"))
import open3dpypro as o3p  # noqa: E402
from open3dpypro import las_io, ops, synthetic as S  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10_000_000)
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--dir", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
n, FMT, STRIDE = args.n, 3, 34
SC, OF = (1e-3,) * 3, S.LAS_OFFSET


def timed(fn, reps=args.reps, sync=True):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3), round(min(ts), 3)


g = torch.Generator(device="cpu").manual_seed(0)
pts = (torch.rand((n, 3), generator=g, dtype=torch.float64) * torch.tensor([40.0, 32.0, 24.0], dtype=torch.float64)
       + torch.tensor(OF, dtype=torch.float64)).to(dev)
col = torch.rand((n, 3), generator=g).to(dev)
inten = torch.randint(-32768, 32767, (n,), generator=g, dtype=torch.int16).to(dev)
cls = torch.randint(0, 256, (n,), generator=g, dtype=torch.uint8).to(dev)

rec, stats = ops.las_pack(pts, STRIDE, FMT, SC, OF, rgb=col, intensity=inten, labels=cls)
torch.cuda.synchronize()
pack_bytes = n * (STRIDE + 24 + 12 + 2 + 1)
med, best = timed(lambda: ops.las_pack(pts, STRIDE, FMT, SC, OF, rgb=col, intensity=inten, labels=cls))
print(json.dumps({"what": "o3dx_las_pack (f64 xyz + rgb + intensity + labels -> records)", "n": n, "median_ms": med,
                  "min_ms": best, "GB_per_s": round(pack_bytes / med / 1e6, 1)}), flush=True)
med, best = timed(lambda: ops.las_pack(pts, STRIDE, FMT, SC, OF))
print(json.dumps({"what": "o3dx_las_pack (f64 xyz -> records)", "n": n, "median_ms": med, "min_ms": best,
                  "GB_per_s": round(n * (STRIDE + 24) / med / 1e6, 1)}), flush=True)
raw = rec.view(-1)
unpack_bytes = n * (STRIDE + 24 + 12 + 12 + 2 + 1)
med, best = timed(lambda: ops.las_unpack(raw, n, STRIDE, FMT, SC, OF, rgb=True, intensity=True, labels=True))
print(json.dumps({"what": "o3dx_las_unpack (records -> f64 + f32 xyz, rgb, intensity, labels)", "n": n,
                  "median_ms": med, "min_ms": best, "GB_per_s": round(unpack_bytes / med / 1e6, 1)}), flush=True)
med, best = timed(lambda: ops.las_unpack(raw, n, STRIDE, FMT, SC, OF))
print(json.dumps({"what": "o3dx_las_unpack (records -> f64 + f32 xyz)", "n": n, "median_ms": med, "min_ms": best,
                  "GB_per_s": round(n * (STRIDE + 36) / med / 1e6, 1)}), flush=True)

with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
    path = os.path.join(tmp, "scan.las")
    las_io.write_file(path, las_io.build_header(FMT, STRIDE, n, SC, OF, stats.cpu().numpy()), rec.cpu().numpy())
    del rec, raw, pts, col, inten, cls
    h = las_io.read_header(path)
    reps = max(3, args.reps // 2)
    med, best = timed(lambda: o3p.PointCloud().read_las(path, rgb=True, intensity=True, labels=True), reps)
    print(json.dumps({"what": "PointCloud.read_las(rgb, intensity, labels), GPU path, file in the page cache", "n": n,
                      "file_MB": round(os.path.getsize(path) / 1e6, 1), "median_ms": med, "min_ms": best}), flush=True)
    med, best = timed(lambda: o3p.PointCloud().read_las(path), reps)
    print(json.dumps({"what": "PointCloud.read_las(), points only, GPU path", "n": n, "median_ms": med,
                      "min_ms": best}), flush=True)

    def host_path():
        d = las_io.decode_host(las_io.read_records(h), h, True, True, True)
        return o3p.PointCloud(d["points"], rgb=d["rgb"], intensity=d["intensity"], labels=d["labels"])

    med, best = timed(host_path, 3)
    print(json.dumps({"what": "the same file through the host numpy path (decode_host + PointCloud(...): its "
                      "float32 check and upload included)", "n": n, "median_ms": med, "min_ms": best,
                      "host_cpus": os.cpu_count()}), flush=True)
    med, best = timed(lambda: las_io.decode_host(las_io.read_records(h), h, True, True, True), 3)
    print(json.dumps({"what": "host numpy decode alone (file read + decode_host)", "n": n, "median_ms": med,
                      "min_ms": best}), flush=True)
    med, best = timed(lambda: las_io.read_records(h), reps, sync=False)
    print(json.dumps({"what": "part: file read (np.fromfile, page cache)", "median_ms": med, "min_ms": best}),
          flush=True)
    buf = las_io.read_records(h)
    med, best = timed(lambda: torch.from_numpy(buf).to(dev), reps)
    print(json.dumps({"what": "part: host-to-device copy of the records (pageable)", "median_ms": med,
                      "min_ms": best, "GB_per_s": round(buf.size / med / 1e6, 1)}), flush=True)
    on_dev = torch.from_numpy(buf).to(dev)

    def decode():
        d = ops.las_unpack(on_dev, n, STRIDE, FMT, SC, OF, rgb=True, intensity=True, labels=True)
        d["flags"].item()
        d["intensity"].cpu(), d["labels"].cpu()

    med, best = timed(decode, reps)
    print(json.dumps({"what": "part: decode call + flag read + intensity / labels back to the host",
                      "median_ms": med, "min_ms": best}), flush=True)
    del on_dev, buf
    c = o3p.PointCloud().read_las(path, rgb=True, intensity=True, labels=True)
    out = os.path.join(tmp, "out.las")
    med, best = timed(lambda: c.save_las(out, scales=SC, offsets=OF, float32_coords=False), 3)
    print(json.dumps({"what": "PointCloud.save_las (GPU pack, records to the host, file write)", "n": n,
                      "median_ms": med, "min_ms": best}), flush=True)
