"""numpy restatement of LAS 1.0-1.4 (uncompressed) for the tests: the public
header through `struct`, the records through one structured dtype per point
format (the ASPRS field tables), and a writer that can produce the layouts the
tests need (extra bytes, a VLR before the points, a 1.4 header with legacy
count 0, bytes after the point block).  Independent of open3dpypro/las_io.py:
it imports nothing from the package."""
import struct

import numpy as np

_HEAD = [("X", "<i4"), ("Y", "<i4"), ("Z", "<i4"), ("intensity", "<u2")]
_LEGACY = _HEAD + [("bits", "u1"), ("classification", "u1"), ("scan_angle_rank", "i1"), ("user_data", "u1"),
                   ("point_source_id", "<u2")]
_MODERN = _HEAD + [("bits", "u1"), ("flags", "u1"), ("classification", "u1"), ("user_data", "u1"),
                   ("scan_angle", "<i2"), ("point_source_id", "<u2"), ("gps_time", "<f8")]
_GPS = [("gps_time", "<f8")]
_RGB = [("red", "<u2"), ("green", "<u2"), ("blue", "<u2")]
_NIR = [("nir", "<u2")]
_WAVE = [("wave_index", "u1"), ("wave_offset", "<u8"), ("wave_size", "<u4"), ("wave_location", "<f4"),
         ("wave_xt", "<f4"), ("wave_yt", "<f4"), ("wave_zt", "<f4")]
FIELDS = {0: _LEGACY, 1: _LEGACY + _GPS, 2: _LEGACY + _RGB, 3: _LEGACY + _GPS + _RGB, 4: _LEGACY + _GPS + _WAVE,
          5: _LEGACY + _GPS + _RGB + _WAVE, 6: _MODERN, 7: _MODERN + _RGB, 8: _MODERN + _RGB + _NIR,
          9: _MODERN + _WAVE, 10: _MODERN + _RGB + _NIR + _WAVE}
MIN_LEN = {f: np.dtype(v).itemsize for f, v in FIELDS.items()}
assert MIN_LEN == {0: 20, 1: 28, 2: 26, 3: 34, 4: 57, 5: 63, 6: 30, 7: 36, 8: 38, 9: 59, 10: 67}
HAS_RGB = {f: any(n == "red" for n, _ in v) for f, v in FIELDS.items()}


def record_dtype(fmt: int, stride: int = None) -> np.dtype:
    fields = list(FIELDS[fmt])
    extra = 0 if stride is None else stride - MIN_LEN[fmt]
    assert extra >= 0
    if extra:
        fields.append(("extra", "u1", (extra,)))
    dt = np.dtype(fields)
    assert dt.itemsize == (stride or MIN_LEN[fmt])
    return dt


def quantise(points, scales, offsets) -> np.ndarray:
    """(n,3) int64 X = np.round((x - offset) / scale) in float64."""
    p = np.asarray(points).astype(np.float64)
    return np.round((p - np.asarray(offsets, np.float64)) / np.asarray(scales, np.float64)).astype(np.int64)


def real(X, scales, offsets) -> np.ndarray:
    return np.asarray(X).astype(np.float64) * np.asarray(scales, np.float64) + np.asarray(offsets, np.float64)


def read_header(b: bytes) -> dict:
    assert b[:4] == b"LASF"
    major, minor = struct.unpack_from("<BB", b, 24)
    day, year, header_size, data_offset, n_vlr = struct.unpack_from("<HHHII", b, 90)
    fmt, stride, legacy = struct.unpack_from("<BHI", b, 104)
    by_return = struct.unpack_from("<5I", b, 111)
    scales = np.array(struct.unpack_from("<3d", b, 131))
    offsets = np.array(struct.unpack_from("<3d", b, 155))
    maxx, minx, maxy, miny, maxz, minz = struct.unpack_from("<6d", b, 179)
    count = legacy
    if (major, minor) >= (1, 4):
        count64, = struct.unpack_from("<Q", b, 247)
        if legacy == 0:
            count = count64
    return {"version": (major, minor), "system_id": b[26:58].rstrip(b"\0").decode(),
            "software": b[58:90].rstrip(b"\0").decode(), "day": day, "year": year, "header_size": header_size,
            "data_offset": data_offset, "n_vlr": n_vlr, "format": fmt, "stride": stride, "legacy_count": legacy,
            "count": count, "by_return": by_return, "scales": scales, "offsets": offsets,
            "mins": np.array([minx, miny, minz]), "maxs": np.array([maxx, maxy, maxz])}


def read(path: str) -> dict:
    """Header fields plus: records (structured), X (n,3) int32, points (n,3)
    float64, rgb (n,3) float32 or None, intensity (n,1) uint16, labels (n,1)
    uint8, tail (the bytes after the point block)."""
    with open(path, "rb") as f:
        b = f.read()
    h = read_header(b)
    dt = record_dtype(h["format"], h["stride"])
    n = h["count"]
    rec = np.frombuffer(b, dtype=dt, count=n, offset=h["data_offset"])
    X = np.stack([rec["X"], rec["Y"], rec["Z"]], 1).astype(np.int32).reshape(n, 3)
    h.update(records=rec, X=X, points=real(X, h["scales"], h["offsets"]),
             intensity=rec["intensity"].astype(np.uint16).reshape(n, 1),
             labels=rec["classification"].astype(np.uint8).reshape(n, 1), rgb=None,
             record_bytes=b[h["data_offset"]:h["data_offset"] + n * h["stride"]],
             tail=b[h["data_offset"] + n * h["stride"]:])
    if HAS_RGB[h["format"]]:
        c = np.stack([rec["red"], rec["green"], rec["blue"]], 1).reshape(n, 3)
        h["rgb"] = (c.astype(np.float64) / 65536.0).astype(np.float32)
    return h


def make_records(fmt: int, X, stride: int = None, rgb16=None, intensity=None, labels=None, fill: int = 0) -> np.ndarray:
    """Structured records; `fill` goes into every byte that is not one of the
    fields above (the decoder must not look at them)."""
    X = np.asarray(X).reshape(-1, 3)
    n = len(X)
    dt = record_dtype(fmt, stride)
    rec = np.frombuffer(bytes([fill]) * (n * dt.itemsize), dtype=dt).copy()
    rec["X"], rec["Y"], rec["Z"] = X[:, 0], X[:, 1], X[:, 2]
    rec["intensity"] = 0 if intensity is None else np.asarray(intensity).reshape(n)
    rec["classification"] = 0 if labels is None else np.asarray(labels).reshape(n)
    if HAS_RGB[fmt]:
        c = np.zeros((n, 3), np.uint16) if rgb16 is None else np.asarray(rgb16).reshape(n, 3)
        rec["red"], rec["green"], rec["blue"] = c[:, 0], c[:, 1], c[:, 2]
    return rec


def minmax(X, scales, offsets):
    X = np.asarray(X).reshape(-1, 3)
    if len(X) == 0:
        return np.zeros(3), np.zeros(3)
    return real(X.min(0), scales, offsets), real(X.max(0), scales, offsets)


def write(path: str, fmt: int, records: np.ndarray, scales, offsets, version=(1, 2), legacy_zero: bool = False,
          vlr_payload: bytes = None, tail: bytes = b"", fmt_byte: int = None, count: int = None):
    """records: make_records' output.  version (1,4) writes the 375-byte header
    (legacy_zero: legacy count 0, the count only in the u64 field);
    vlr_payload: one VLR (54-byte header + payload) between header and points;
    tail: bytes after the point block; fmt_byte / count: override the header's
    point-format byte / point count (for the rejection tests)."""
    n = len(records)
    count = n if count is None else count
    header_size = 375 if tuple(version) >= (1, 4) else (235 if tuple(version) == (1, 3) else 227)
    vlr = b""
    if vlr_payload is not None:
        vlr = struct.pack("<H16sHH32s", 0, b"oracle", 7, len(vlr_payload), b"test record") + vlr_payload
        assert len(vlr) == 54 + len(vlr_payload)
    X = np.stack([records["X"], records["Y"], records["Z"]], 1).reshape(n, 3)
    mins, maxs = minmax(X, scales, offsets)
    b = bytearray(header_size)
    b[0:4] = b"LASF"
    struct.pack_into("<BB", b, 24, *version)
    struct.pack_into("<32s32s", b, 26, b"OTHER", b"las_oracle")
    struct.pack_into("<HHHII", b, 90, 1, 2024, header_size, header_size + len(vlr), 1 if vlr else 0)
    struct.pack_into("<BHI", b, 104, fmt if fmt_byte is None else fmt_byte, records.dtype.itemsize,
                     0 if legacy_zero else count)
    struct.pack_into("<3d", b, 131, *np.asarray(scales, np.float64))
    struct.pack_into("<3d", b, 155, *np.asarray(offsets, np.float64))
    struct.pack_into("<6d", b, 179, maxs[0], mins[0], maxs[1], mins[1], maxs[2], mins[2])
    if header_size == 375:
        struct.pack_into("<Q", b, 247, count)
    with open(path, "wb") as f:
        f.write(bytes(b) + vlr + records.tobytes() + tail)
