"""LAS (ASPRS LAS 1.0-1.4, uncompressed) reader/writer without laspy.

Replaces laspy behind PointCloudAdvanceIO.read_las / read_las_gen / save_las /
append_save_las (reference open3dpypro/PointCloud.py:496-567).  As with PCD
(pcd_io.py) the public header is parsed and written
here, on the host; the record block travels between the file and HBM in one
copy and every record is decoded / encoded by a kernel (csrc/las.hip:
o3dx_las_unpack, o3dx_las_pack).  decode_host / pack_host are the numpy forms
of the same rules with identical values, for machines without a GPU.

Public header, little-endian: signature "LASF" at 0, version major / minor at
24 / 25, system id at 26 (32 bytes), generating software at 58 (32), creation
day of year / year u16 at 90 / 92, header size u16 at 94, offset to point data
u32 at 96, number of VLRs u32 at 100, point format u8 at 104, record length
u16 at 105, legacy point count u32 at 107, legacy by-return counts 5 x u32 at
111, scales 3 x f64 at 131, offsets 3 x f64 at 155, max x, min x, max y,
min y, max z, min z (f64) at 179; LAS 1.4 adds the u64 point count at 247,
used when the legacy count is 0.  VLRs are skipped: the points start at
"offset to point data".  The record stride is the header's record length; it
may exceed the format's minimum (extra bytes).

Rules (include/o3dx.h "LAS IO" states them for the kernels):
  x = X * scale + offset in float64, one multiply then one add;
  colour = u16 / 65536 (exact in float32); intensity = the raw u16;
  labels = the whole classification byte: offset 15 in formats 0-5 (laspy's
  raw_classification), offset 16 in formats 6-10 (this project's rule: laspy
  has no raw_classification there);
  writing: X = np.round((x - offset) / scale) in float64 (ties to even);
  colour (uint8)(c * 255.0) stored in the u16 field, as the reference's
  get_lasdata does — reading it back through / 65536 dims it 256-fold.
Compressed LAZ (bit 6 or 7 of the point-format byte) is rejected.
"""
from __future__ import annotations

import datetime
import os
import struct

import numpy as np

SOFTWARE = "open3dpypro-mi355x"
SYSTEM_ID = "OTHER"
# point format -> (minimal record length, classification byte, offset of red/green/blue or None);
# X, Y, Z int32 at 0, 4, 8 and the intensity u16 at 12 in every format
LAYOUT = {0: (20, 15, None), 1: (28, 15, None), 2: (26, 15, 20), 3: (34, 15, 28), 4: (57, 15, None),
          5: (63, 15, 28), 6: (30, 16, None), 7: (36, 16, 30), 8: (38, 16, 30), 9: (59, 16, None),
          10: (67, 16, 30)}
WRITABLE = (0, 1, 2, 3, 6, 7, 8)  # the formats o3dx_las_pack / pack_host write
HEADER_12 = 227
HEADER_14 = 375
_I32_MIN, _I32_MAX = -2147483648, 2147483647


class LasHeader:
    """The public-header fields this package uses."""

    def __init__(self, path, version, header_size, data_offset, point_format, stride, count, legacy_count, scales,
                 offsets, mins, maxs, file_size):
        self.path = path
        self.version = version            # (major, minor)
        self.header_size = header_size
        self.data_offset = data_offset    # offset to point data
        self.point_format = point_format
        self.stride = stride              # record length
        self.count = count                # point count (legacy, or the 1.4 u64 count)
        self.legacy_count = legacy_count
        self.scales = scales              # (3,) float64
        self.offsets = offsets
        self.mins = mins
        self.maxs = maxs
        self.file_size = file_size

    @property
    def has_rgb(self) -> bool:
        return LAYOUT[self.point_format][2] is not None


def read_header(path: str) -> LasHeader:
    """Parse and validate the public header; RuntimeError names the file and the reason."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        b = f.read(HEADER_14)
    if b[:4] != b"LASF":
        raise RuntimeError(f"{path}: not a LAS file (bad signature {b[:4]!r})")
    if len(b) < HEADER_12:
        raise RuntimeError(f"{path}: truncated LAS header ({len(b)} bytes)")
    version = (b[24], b[25])
    header_size, data_offset = struct.unpack_from("<HI", b, 94)
    fmt_byte = b[104]
    stride, = struct.unpack_from("<H", b, 105)
    legacy, = struct.unpack_from("<I", b, 107)
    if fmt_byte & 0xC0:
        raise RuntimeError(f"{path}: compressed LAZ point data (point-format byte {fmt_byte:#04x}) is not supported")
    if fmt_byte > 10:
        raise RuntimeError(f"{path}: unknown point format {fmt_byte} (0..10)")
    if stride < LAYOUT[fmt_byte][0]:
        raise RuntimeError(f"{path}: record length {stride} is below the {LAYOUT[fmt_byte][0]} bytes of point "
                           f"format {fmt_byte}")
    count = legacy
    if legacy == 0 and version >= (1, 4) and header_size >= HEADER_14 and len(b) >= HEADER_14:
        count, = struct.unpack_from("<Q", b, 247)
    if data_offset < max(header_size, HEADER_12):
        raise RuntimeError(f"{path}: offset to point data {data_offset} lies inside the {header_size}-byte header")
    if size - data_offset < count * stride:
        raise RuntimeError(f"{path}: point data is shorter than {count} records x {stride} bytes "
                           f"({max(size - data_offset, 0)} bytes follow the header)")
    sc = np.array(struct.unpack_from("<3d", b, 131), np.float64)
    of = np.array(struct.unpack_from("<3d", b, 155), np.float64)
    mm = struct.unpack_from("<6d", b, 179)
    return LasHeader(path, version, header_size, data_offset, fmt_byte, stride, count, legacy, sc, of,
                     np.array(mm[1::2], np.float64), np.array(mm[0::2], np.float64), size)


def read_records(h: LasHeader, start: int = 0, count: int = None) -> np.ndarray:
    """Records [start, start + count) of the file as one uint8 array (count * stride,)."""
    count = h.count - start if count is None else count
    with open(h.path, "rb") as f:
        f.seek(h.data_offset + start * h.stride)
        raw = np.fromfile(f, dtype=np.uint8, count=count * h.stride)
    if raw.size != count * h.stride:
        raise RuntimeError(f"{h.path}: point data is shorter than the header's count")
    return raw


def decode_host(raw: np.ndarray, h: LasHeader, rgb: bool = False, intensity: bool = False, labels: bool = False):
    """numpy decode of a record block: the values o3dx_las_unpack produces."""
    _, cls_off, rgb_off = LAYOUT[h.point_format]
    n = raw.size // h.stride
    rec = raw.reshape(n, h.stride)
    X = np.ascontiguousarray(rec[:, :12]).view("<i4")
    out = {"points": X.astype(np.float64) * h.scales + h.offsets, "rgb": None, "intensity": None, "labels": None}
    if rgb:
        c = np.ascontiguousarray(rec[:, rgb_off:rgb_off + 6]).view("<u2")
        out["rgb"] = c.astype(np.float32) / np.float32(65536.0)
    if intensity:
        out["intensity"] = np.ascontiguousarray(rec[:, 12:14]).view("<u2").astype(np.uint16).reshape(n, 1)
    if labels:
        out["labels"] = np.ascontiguousarray(rec[:, cls_off:cls_off + 1]).reshape(n, 1)
    return out


def decode_device(raw: np.ndarray, h: LasHeader, device, rgb: bool = False, intensity: bool = False,
                  labels: bool = False):
    """The record block goes to the device in one copy and is decoded there
    (ops.las_unpack); device tensors, intensity / labels as (n,1) numpy."""
    import torch

    from . import ops

    n = raw.size // h.stride
    d = ops.las_unpack(torch.from_numpy(raw).to(device), n, h.stride, h.point_format, h.scales, h.offsets, rgb=rgb,
                       intensity=intensity, labels=labels)
    wide = bool(int(d["flags"].item()) & 1)
    return {"points32": d["points32"], "points64": d["points64"] if wide else None, "wide": wide, "rgb": d["rgb"],
            "intensity": d["intensity"].cpu().numpy().view(np.uint16).reshape(n, 1) if intensity else None,
            "labels": d["labels"].cpu().numpy().reshape(n, 1) if labels else None}


def pack_host(points: np.ndarray, point_format: int, stride: int, scales, offsets, rgb=None, intensity=None,
              labels=None):
    """numpy encode: (records (n, stride) uint8, stats (8,) int64), the values
    o3dx_las_pack produces.  points (n,3) float32 or float64; rgb (n,3)
    float32; intensity (n,) uint16; labels (n,) uint8."""
    min_len, cls_off, rgb_off = LAYOUT[point_format]
    n = len(points)
    sc, of = np.asarray(scales, np.float64).reshape(3), np.asarray(offsets, np.float64).reshape(3)
    with np.errstate(all="ignore"):
        q = np.round((np.asarray(points).astype(np.float64).reshape(n, 3) - of) / sc)
        bad = ~np.isfinite(q)
        over = ~bad & ((q < float(_I32_MIN)) | (q > float(_I32_MAX)))
        ok = ~(bad | over)
        X = np.where(ok, q, 0.0).astype("<i4")
    stats = np.zeros(8, np.int64)
    for a in range(3):
        v = X[ok[:, a], a]
        stats[a] = v.min() if v.size else _I32_MAX
        stats[3 + a] = v.max() if v.size else _I32_MIN
    stats[6], stats[7] = int(over.sum()), int(bad.sum())
    rec = np.zeros((n, stride), np.uint8)
    rec[:, :12] = X.view(np.uint8).reshape(n, 12)
    if intensity is not None:
        rec[:, 12:14] = np.ascontiguousarray(intensity, "<u2").reshape(n, 1).view(np.uint8)
    if labels is not None:
        rec[:, cls_off] = np.asarray(labels, np.uint8).reshape(n)
    if rgb is not None:
        with np.errstate(all="ignore"):
            c = (np.asarray(rgb).astype(np.float64).reshape(n, 3) * 255.0).astype(np.uint8)
        rec[:, rgb_off:rgb_off + 6] = np.ascontiguousarray(c.astype("<u2")).view(np.uint8)
    return rec, stats


def _real(stats_int: np.ndarray, scales, offsets) -> np.ndarray:
    return np.asarray(stats_int, np.float64) * scales + offsets


def check_stats(stats: np.ndarray, what: str):
    """ValueError for non-finite coordinates (this project's rule), OverflowError
    when a scaled coordinate leaves int32 (laspy raises the same type)."""
    if stats[7]:
        raise ValueError(f"{what}: {int(stats[7])} coordinate values are not finite")
    if stats[6]:
        raise OverflowError(f"{what}: {int(stats[6])} coordinate values do not fit int32 after (x - offset) / scale; "
                            "choose a larger scale or suitable offsets")


def build_header(point_format: int, stride: int, n: int, scales, offsets, stats: np.ndarray,
                 today: datetime.date = None) -> bytes:
    """A LAS 1.2 public header (227 bytes, no VLRs): what laspy writes for
    LasHeader(point_format, version="1.2") — by-return counts all 0 (return
    number 0 is not counted)."""
    if n >= 1 << 32:
        raise RuntimeError("a LAS 1.2 header holds at most 2^32 - 1 points")
    today = today or datetime.date.today()
    sc, of = np.asarray(scales, np.float64).reshape(3), np.asarray(offsets, np.float64).reshape(3)
    mins = _real(stats[0:3], sc, of) if n else np.zeros(3)
    maxs = _real(stats[3:6], sc, of) if n else np.zeros(3)
    b = bytearray(HEADER_12)
    b[0:4] = b"LASF"
    b[24], b[25] = 1, 2
    b[26:26 + len(SYSTEM_ID)] = SYSTEM_ID.encode("ascii")
    b[58:58 + len(SOFTWARE)] = SOFTWARE.encode("ascii")
    struct.pack_into("<HHHI", b, 90, today.timetuple().tm_yday, today.year, HEADER_12, HEADER_12)
    struct.pack_into("<I", b, 100, 0)
    b[104] = point_format
    struct.pack_into("<H", b, 105, stride)
    struct.pack_into("<I", b, 107, n)
    struct.pack_into("<3d", b, 131, *sc)
    struct.pack_into("<3d", b, 155, *of)
    struct.pack_into("<6d", b, 179, maxs[0], mins[0], maxs[1], mins[1], maxs[2], mins[2])
    return bytes(b)


def write_file(path: str, header: bytes, records: np.ndarray):
    with open(path, "wb") as f:
        f.write(header)
        np.ascontiguousarray(records).tofile(f)


def check_appendable(h: LasHeader):
    if h.point_format not in WRITABLE:
        raise RuntimeError(f"{h.path}: point format {h.point_format} cannot be written (only {WRITABLE})")
    end = h.data_offset + h.count * h.stride
    if h.file_size != end:
        raise RuntimeError(f"{h.path}: {h.file_size - end} bytes follow the point block (EVLRs); appending would "
                           "overwrite them")


def append_records(h: LasHeader, records: np.ndarray, stats: np.ndarray):
    """Append packed records to the file of `h` and rewrite the count(s) and
    the merged min / max."""
    n = len(records)
    if n == 0:
        return
    total = h.count + n
    use_legacy = h.version < (1, 4) or h.legacy_count != 0 or h.header_size < HEADER_14
    if use_legacy and total >= 1 << 32:
        raise RuntimeError(f"{h.path}: {total} points do not fit the legacy point count")
    mins, maxs = _real(stats[0:3], h.scales, h.offsets), _real(stats[3:6], h.scales, h.offsets)
    if h.count:
        mins, maxs = np.minimum(mins, h.mins), np.maximum(maxs, h.maxs)
    with open(h.path, "r+b") as f:
        f.seek(h.data_offset + h.count * h.stride)
        np.ascontiguousarray(records).tofile(f)
        if use_legacy:
            f.seek(107)
            f.write(struct.pack("<I", total))
        if h.version >= (1, 4) and h.header_size >= HEADER_14:
            f.seek(247)
            f.write(struct.pack("<Q", total))
        f.seek(179)
        f.write(struct.pack("<6d", maxs[0], mins[0], maxs[1], mins[1], maxs[2], mins[2]))
