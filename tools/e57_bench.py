"""E57 kernel speed (GPU box only; reads no file it did not write).  A
self-written scan of --n points (float64 georeferenced x y z, float32
intensity, colours, 13-bit row and 12-bit column indices):
  1. o3dx_e57_pack, o3dx_e57_seal, o3dx_e57_crc_pages and o3dx_e57_unpack on
     bytes already on the device: a host clock around synchronised calls (the
     wrapper's allocations and table uploads included), the median of --reps
     calls after a warm-up, the bytes each call moves over that time, and the
     kernel alone by the library's event timing (kernel_ms);
  2. in the same run a device-to-device copy of the file's byte count, and each
     kernel's time as a factor of it;
  3. the numpy host forms (pack_host, seal_host, crc32c_pages_host,
     decode_host) on --host-n points.
Every line goes to stdout and to --out.
Usage: python tools/e57_bench.py [--n 10000000] [--host-n 1000000] [--reps 11] [--out profiles/e57_kernels.txt]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "open3d-py-extension_amd"))
from open3dpypro import _native as N, e57_io as S, ops, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10_000_000)
ap.add_argument("--host-n", type=int, default=1_000_000)
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "e57_kernels.txt"))
args = ap.parse_args()
dev = torch.device("cuda:0")
N.set_kernel_timing(True)
lines = []


def emit(rec):
    line = json.dumps(rec)
    lines.append(line)
    print(line, flush=True)


def timed(fn, reps=args.reps, sync=True):
    fn()  # warm-up
    N.reset_kernel_timing()
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


def kernel_ms(name):
    """The library's own event timing of the kernel alone, mean over the timed calls."""
    torch.cuda.synchronize()
    ms, launches = N.kernel_timing(name)
    return round(ms / max(launches, 1), 3)


def make(n, device):
    g = torch.Generator(device="cpu").manual_seed(0)
    pts = torch.rand((n, 3), generator=g, dtype=torch.float64) * torch.tensor([40.0, 32.0, 24.0], dtype=torch.float64) \
        + torch.tensor(synthetic.LAS_OFFSET, dtype=torch.float64)
    inten = torch.rand(n, generator=g) * 4096.0
    col = torch.rand((n, 3), generator=g)
    row = torch.randint(0, 8192, (n,), generator=g, dtype=torch.int64)
    column = torch.randint(0, 4096, (n,), generator=g, dtype=torch.int64)
    fields = [(k, S.SRC_F64, 64, 0, 0) for k in ("cartesianX", "cartesianY", "cartesianZ")]
    fields += [("intensity", S.SRC_F32, 32, 0, 0)]
    fields += [(k, S.SRC_COLOUR, 8, 0, 255) for k in ("colorRed", "colorGreen", "colorBlue")]
    fields += [("rowIndex", S.SRC_I64, 13, 0, 8191), ("columnIndex", S.SRC_I64, 12, 0, 4095)]
    kinds = ["double"] * 3 + ["single"] + [(0, 255)] * 3 + [(0, 8191), (0, 4095)]
    if device is None:
        p, c = pts.numpy(), col.numpy()
        cols = [p[:, 0], p[:, 1], p[:, 2], inten.numpy(), c[:, 0], c[:, 1], c[:, 2], row.numpy(), column.numpy()]
    else:
        p, c = pts.to(device), col.to(device)
        cols = [(p, 3, 0), (p, 3, 1), (p, 3, 2), (inten.to(device), 1, 0), (c, 3, 0), (c, 3, 1), (c, 3, 2),
                (row.to(device), 1, 0), (column.to(device), 1, 0)]
    return S.ScanPlan(fields, n), kinds, cols


def image_parts(plan, kinds):
    (sec,), xml_at = S.layout([plan])
    xml = S.file_xml([S.scan_xml(plan, S.physical(sec), "bench", "{bench}", None, None, None, None, kinds)], False)
    size = (xml_at + len(xml) + 3) // 4 * 4
    return sec, xml_at, xml, size


n = args.n
plan, kinds, cols = make(n, dev)
sec, xml_at, xml, size = image_parts(plan, kinds)
src_bytes = n * (24 + 4 + 12 + 16)
image = torch.zeros(size, dtype=torch.uint8, device=dev)
image[:48] = torch.from_numpy(np.frombuffer(S.file_header(xml_at, len(xml)), np.uint8).copy()).to(dev)
image[sec:sec + 32] = torch.from_numpy(np.frombuffer(S.section_header(plan, sec), np.uint8).copy()).to(dev)
image[xml_at:xml_at + len(xml)] = torch.from_numpy(np.frombuffer(xml, np.uint8).copy()).to(dev)
body = image[sec + 32:sec + 32 + plan.data_bytes]


def pack():
    ops.e57_pack(plan.tables(), cols, plan.n, plan.R, plan.full_bytes, plan.last_bytes, plan.packet_head(False),
                 plan.packet_head(True), out=body)


emit({"what": "file", "n": n, "packets": plan.packets, "records_per_packet": plan.R, "logical_bytes": size,
      "source_bytes": src_bytes})
med, best = timed(pack)
t_pack = med
emit({"what": "o3dx_e57_pack (9 columns -> packets)", "median_ms": med, "min_ms": best,
      "kernel_ms": kernel_ms("e57_pack"),
      "GB_per_s": round((src_bytes + plan.data_bytes) / med / 1e6, 1)})
paged = ops.e57_seal(image)
med, best = timed(lambda: ops.e57_seal(image))
t_seal = med
emit({"what": "o3dx_e57_seal (logical -> pages + CRC trailers)", "median_ms": med, "min_ms": best,
      "kernel_ms": kernel_ms("e57_seal"),
      "GB_per_s": round((size + paged.numel()) / med / 1e6, 1)})
assert ops.e57_crc_pages(paged) == (0, -1)
med, best = timed(lambda: ops.e57_crc_pages(paged))
t_crc = med
emit({"what": "o3dx_e57_crc_pages (whole file; includes the 16-byte result read)", "median_ms": med, "min_ms": best,
      "kernel_ms": kernel_ms("e57_crc_pages"),
      "GB_per_s": round(paged.numel() / med / 1e6, 1)})
raw = paged.cpu().numpy()
hdr = S.read_header(raw, "bench")
fields = S.wanted_fields(hdr.scans[0], rgb=True, intensity=True, row_column=True)
desc, aff, segs = S.field_tables(fields)
d = ops.e57_unpack(paged, desc, aff, segs, 0, n)
assert int(d["flags"].item()) == S.FLAG_NOT_F32 and torch.equal(d["points64"], cols[0][0])
out_bytes = n * (24 + 12 + 3 + 4 + 2 + 2)
med, best = timed(lambda: ops.e57_unpack(paged, desc, aff, segs, 0, n))
t_unpack = med
emit({"what": "o3dx_e57_unpack (f64 + f32 xyz, rgb, intensity, row, column; segment table upload included)",
      "median_ms": med, "min_ms": best, "kernel_ms": kernel_ms("e57_unpack"),
      "GB_per_s": round((plan.data_bytes + out_bytes) / med / 1e6, 1)})
dst = torch.empty_like(paged)
med, best = timed(lambda: dst.copy_(paged))
emit({"what": "device-to-device copy of the file's bytes", "bytes": paged.numel(), "median_ms": med, "min_ms": best,
      "GB_per_s": round(2 * paged.numel() / med / 1e6, 1)})
emit({"what": "factor of the copy's time", "pack": round(t_pack / med, 2), "seal": round(t_seal / med, 2),
      "crc_pages": round(t_crc / med, 2), "unpack": round(t_unpack / med, 2)})
del d, dst, image, body, paged, cols

hn = args.host_n
plan, kinds, cols = make(hn, None)
sec, xml_at, xml, size = image_parts(plan, kinds)
med, best = timed(lambda: S.pack_host(plan, cols), 3, sync=False)
emit({"what": "pack_host (numpy)", "n": hn, "median_ms": med, "min_ms": best, "host_cpus": os.cpu_count()})
lg = np.zeros(size, np.uint8)
lg[:48] = np.frombuffer(S.file_header(xml_at, len(xml)), np.uint8)
lg[sec:sec + 32] = np.frombuffer(S.section_header(plan, sec), np.uint8)
lg[sec + 32:sec + 32 + plan.data_bytes] = S.pack_host(plan, cols)
lg[xml_at:xml_at + len(xml)] = np.frombuffer(xml, np.uint8)
med, best = timed(lambda: S.seal_host(lg), 3, sync=False)
emit({"what": "seal_host (numpy)", "n": hn, "bytes": size, "median_ms": med, "min_ms": best})
raw = S.seal_host(lg)
med, best = timed(lambda: S.crc32c_pages_host(raw), 3, sync=False)
emit({"what": "crc32c_pages_host (numpy)", "n": hn, "bytes": raw.size, "median_ms": med, "min_ms": best})
fields = S.wanted_fields(S.read_header(raw, "bench").scans[0], rgb=True, intensity=True, row_column=True)
med, best = timed(lambda: S.decode_host(raw, fields, 0, hn), 3, sync=False)
emit({"what": "decode_host (numpy)", "n": hn, "median_ms": med, "min_ms": best})
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
