"""E57 (ASTM E2807) reader / writer without pye57 or libE57.

Replaces pye57 behind PointCloudAdvanceIO.read_e57* / save_e57 / save_pcds_e57
/ e572las and the reference's E57File (reference open3dpypro/PointCloud.py:
569-703, open3dpypro/E57File.py).  The host parses the 48-byte file header,
the XML and the packet headers of every scan's section (about 16 per MiB) and
builds, per prototype field, a segment table {stream byte offset, logical file
offset, length}.  The file bytes travel to HBM once; the page checksums, the
record decode and the encode run there (csrc/e57.hip: o3dx_e57_crc_pages,
o3dx_e57_unpack, o3dx_e57_pack, o3dx_e57_seal).  crc32c_pages_host /
decode_host / pack_host / seal_host are the numpy forms of the same rules with
identical values, for machines without a GPU.

Layout, little-endian.  File header: "ASTM-E57", major u32, minor u32,
filePhysicalLength u64, xmlPhysicalOffset u64, xmlLogicalLength u64, pageSize
u64 (1024).  A page is 1020 payload bytes and a big-endian CRC32C (Castagnoli)
of them; every stored offset is physical, logical = physical - 4 * (physical
// 1024).  A scan's points are a CompressedVector section: a 32-byte header
(sectionId 1, 7 reserved, sectionLogicalLength u64, dataPhysicalOffset u64,
indexPhysicalOffset u64), then packets.  A data packet: u8 type 1, u8 flags,
u16 length - 1, u16 bytestreamCount, bytestreamCount u16 stream lengths, then
the streams in prototype order.  Index (type 0) and ignored (type 2) packets
are skipped by their length field.

Rules (include/o3dx.h "E57 IO" states them for the kernels):
  record r of a field of b bits is the b bits from bit r * b of the field's
  bytestream, LSB first, continuous across packets;
  Float single widens to float64 exactly; Integer = minimum + raw (int64);
  ScaledInteger = (double)int64 * scale + offset, one multiply then one add;
  pose (this project's rule; pye57 is absent): R from the quaternion w, x, y, z
  as stored (not normalised) by pose_matrix below, in float64, and
  x' = ((R00 * x + R01 * y) + R02 * z) + t0, in that order;
  writing: packets of a fixed R records, R the largest multiple of 8 whose
  packet is <= 65,536 bytes; colours (uint8)(c * 255.0) as Integer 0..255.
Out of scope: spherical coordinates, images2D, Blob sections, String or nested
prototype fields, index packets on writing.
"""
from __future__ import annotations

import os
import struct
import uuid
import xml.etree.ElementTree as ET
from xml.sax.saxutils import escape

import numpy as np

SIGNATURE = b"ASTM-E57"
PAGE = 1024
PAYLOAD = 1020
HEADER = 48
SECTION_HEADER = 32
MAX_PACKET = 65536
NS = "http://www.astm.org/COMMIT/E57/2010-e57-v1.0"
NS_NOR = "http://www.libe57.org/E57_NOR_surface_normals.txt"
LIBRARY = "open3dpypro-mi355x"
_I64_MIN, _I64_MAX = -(1 << 63), (1 << 63) - 1
_M64 = (1 << 64) - 1

KIND_F32, KIND_F64, KIND_INT, KIND_SCALED = 0, 1, 2, 3
# the roles o3dx_e57_unpack knows (include/o3dx.h O3DX_E57_ROLE_*)
ROLES = {"cartesianX": 0, "cartesianY": 1, "cartesianZ": 2, "intensity": 3, "colorRed": 4, "colorGreen": 5,
         "colorBlue": 6, "rowIndex": 7, "columnIndex": 8, "cartesianInvalidState": 9}
_INT_ROLES = (4, 5, 6, 7, 8, 9)  # decoded into integer columns: Integer fields only
# sources o3dx_e57_pack reads (include/o3dx.h O3DX_E57_SRC_*)
SRC_F32, SRC_F64, SRC_COLOUR, SRC_I64 = 0, 1, 2, 3
FLAG_NOT_F32, FLAG_RANGE = 1, 2


# ------------------------------------------------------------------ checksums
def _make_tables():
    t = np.zeros((8, 256), np.uint32)
    c = np.arange(256, dtype=np.uint32)
    for _ in range(8):
        c = np.where(c & 1, (c >> 1) ^ np.uint32(0x82F63B78), c >> 1).astype(np.uint32)
    t[0] = c
    for k in range(1, 8):
        t[k] = t[0][t[k - 1] & 0xFF] ^ (t[k - 1] >> 8)
    return t


CRC_TABLES = _make_tables()  # slice-by-8 tables; row 0 is the byte table


def crc32c(data) -> int:
    """CRC32C (Castagnoli: reflected 0x82F63B78, init and final xor 0xFFFFFFFF)."""
    crc = 0xFFFFFFFF
    t = CRC_TABLES[0]
    for b in bytes(data):
        crc = int(t[(crc ^ b) & 0xFF]) ^ (crc >> 8)
    return crc ^ 0xFFFFFFFF


def _crc_rows(rows: np.ndarray) -> np.ndarray:
    """CRC32C of every row of a (pages, 1020) uint8 array, all rows at once."""
    crc = np.full(rows.shape[0], 0xFFFFFFFF, np.uint32)
    t = CRC_TABLES[0]
    cols = np.ascontiguousarray(rows.T)
    for k in range(rows.shape[1]):
        crc = t[(crc ^ cols[k]) & 0xFF] ^ (crc >> 8)
    return crc ^ np.uint32(0xFFFFFFFF)


def crc32c_pages_host(raw: np.ndarray):
    """(bad count, first bad page or -1): the values o3dx_e57_crc_pages
    produces, for whole pages of `raw`."""
    pages = raw[:raw.size // PAGE * PAGE].reshape(-1, PAGE)
    if pages.shape[0] == 0:
        return 0, -1
    want = np.ascontiguousarray(pages[:, PAYLOAD:]).view(">u4").reshape(-1)
    bad = np.nonzero(_crc_rows(pages[:, :PAYLOAD]) != want)[0]
    return int(bad.size), int(bad[0]) if bad.size else -1


def seal_host(logical: np.ndarray) -> np.ndarray:
    """Logical bytes laid into 1024-byte pages, each with its CRC trailer (the
    last page zero-padded): the bytes o3dx_e57_seal produces."""
    n_pages = (logical.size + PAYLOAD - 1) // PAYLOAD
    out = np.zeros((n_pages, PAGE), np.uint8)
    body = np.zeros(n_pages * PAYLOAD, np.uint8)
    body[:logical.size] = logical
    out[:, :PAYLOAD] = body.reshape(n_pages, PAYLOAD)
    out[:, PAYLOAD:] = _crc_rows(out[:, :PAYLOAD]).astype(">u4").view(np.uint8).reshape(n_pages, 4)
    return out.reshape(-1)


# -------------------------------------------------------------------- offsets
def physical(logical: int) -> int:
    return logical + 4 * (logical // PAYLOAD)


def logical(phys: int) -> int:
    return phys - 4 * (phys // PAGE)


def _lread(raw: np.ndarray, path: str, off: int, n: int, what: str) -> bytes:
    """n logical bytes from logical offset off (page trailers skipped)."""
    i = off + np.arange(n, dtype=np.int64)
    p = i + 4 * (i // PAYLOAD)
    if n and (off < 0 or int(p[-1]) >= raw.size):
        raise RuntimeError(f"{path}: truncated data ({what} at logical offset {off} needs {n} bytes; the file has "
                           f"{raw.size})")
    return raw[p].tobytes()


# ------------------------------------------------------------------- the model
class E57Field:
    """One prototype field: kind (KIND_*), bits per record, minimum, scale, offset."""

    def __init__(self, name, kind, bits, minimum=0, maximum=0, scale=1.0, offset=0.0):
        self.name = name
        self.kind = kind
        self.bits = bits
        self.minimum = minimum
        self.maximum = maximum
        self.scale = scale
        self.offset = offset
        self.segments = np.zeros((0, 3), np.int64)  # {stream byte offset, logical file offset, length}

    @property
    def role(self) -> int:
        return ROLES.get(self.name, -1)


class ScanHeader:
    """What the reference reads from a pye57 scan header, as plain values."""

    def __init__(self, index):
        self.index = index
        self.name = ""
        self.guid = ""
        self.point_count = 0
        self.fields = []            # E57Field, prototype order
        self.rotation = np.array([1.0, 0.0, 0.0, 0.0])  # w, x, y, z
        self.translation = np.zeros(3)
        self.has_pose = False
        self.cartesianBounds = None  # {xMinimum, xMaximum, ...} floats, or None
        self.intensityLimits = None
        self.section_offset = 0      # physical

    @property
    def point_fields(self):
        return [f.name for f in self.fields]

    def field(self, name):
        for f in self.fields:
            if f.name == name:
                return f
        return None


def pose_matrix(rotation, translation) -> np.ndarray:
    """12 float64: R row-major from the quaternion w, x, y, z as it stands (not
    normalised), then t."""
    w, x, y, z = (float(v) for v in rotation)
    t = [float(v) for v in translation]
    return np.array([1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
                     2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
                     2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y),
                     t[0], t[1], t[2]], np.float64)


# ----------------------------------------------------------------- the XML
def _local(tag: str, prefixes: dict) -> str:
    if tag.startswith("{"):
        uri, name = tag[1:].split("}", 1)
        if uri == NS:
            return name
        return f"{prefixes.get(uri, 'ext')}:{name}"
    return tag


def _number(el, default=0.0):
    if el is None:
        return default
    txt = (el.text or "").strip()
    if el.get("type") == "Integer":
        return int(txt) if txt else 0
    return float(txt) if txt else 0.0


def _child(el, name):
    return None if el is None else el.find(f"{{{NS}}}{name}")


def _parse_field(el, name, path) -> E57Field:
    typ = el.get("type")
    if typ == "Float":
        single = el.get("precision", "double") == "single"
        return E57Field(name, KIND_F32 if single else KIND_F64, 32 if single else 64)
    if typ in ("Integer", "ScaledInteger"):
        mn = int(el.get("minimum", _I64_MIN))
        mx = int(el.get("maximum", _I64_MAX))
        if mx < mn:
            raise RuntimeError(f"{path}: field {name} has maximum {mx} below minimum {mn}")
        bits = (mx - mn).bit_length()
        if typ == "Integer":
            return E57Field(name, KIND_INT, bits, mn, mx)
        return E57Field(name, KIND_SCALED, bits, mn, mx, float(el.get("scale", 1.0)), float(el.get("offset", 0.0)))
    raise RuntimeError(f"{path}: prototype field {name} of type {typ} is not supported (Float, Integer, "
                       "ScaledInteger)")


def parse_xml(xml: bytes, path: str):
    """The data3D scans of the XML section as ScanHeader objects (no segments yet)."""
    import io

    prefixes = {}
    try:
        root = None
        for ev, item in ET.iterparse(io.BytesIO(xml), events=("start-ns", "start")):
            if ev == "start-ns":
                prefixes[item[1]] = item[0]
            elif root is None:
                root = item
    except ET.ParseError as e:
        raise RuntimeError(f"{path}: the XML section does not parse ({e})")
    scans = []
    data3d = _child(root, "data3D")
    for i, sc in enumerate(list(data3d) if data3d is not None else []):
        h = ScanHeader(i)
        h.name = (getattr(_child(sc, "name"), "text", None) or "")
        h.guid = (getattr(_child(sc, "guid"), "text", None) or "")
        pose = _child(sc, "pose")
        if pose is not None:
            h.has_pose = True
            rot, tr = _child(pose, "rotation"), _child(pose, "translation")
            if rot is not None:
                h.rotation = np.array([_number(_child(rot, "w"), 1.0)] + [_number(_child(rot, k)) for k in "xyz"],
                                      np.float64)
            if tr is not None:
                h.translation = np.array([_number(_child(tr, k)) for k in "xyz"], np.float64)
        cb = _child(sc, "cartesianBounds")
        if cb is not None:
            h.cartesianBounds = {k: float(_number(_child(cb, k))) for k in
                                 ("xMinimum", "xMaximum", "yMinimum", "yMaximum", "zMinimum", "zMaximum")}
        il = _child(sc, "intensityLimits")
        if il is not None:
            h.intensityLimits = {k: float(_number(_child(il, k))) for k in ("intensityMinimum", "intensityMaximum")}
        pts = _child(sc, "points")
        if pts is None or pts.get("type") != "CompressedVector":
            raise RuntimeError(f"{path}: scan {i} has no CompressedVector of points")
        h.point_count = int(pts.get("recordCount", 0))
        h.section_offset = int(pts.get("fileOffset", 0))
        proto = _child(pts, "prototype")
        for f in (list(proto) if proto is not None else []):
            h.fields.append(_parse_field(f, _local(f.tag, prefixes), path))
        names = h.point_fields
        if not all(k in names for k in ("cartesianX", "cartesianY", "cartesianZ")):
            if any(k.startswith("spherical") for k in names):
                raise RuntimeError(f"{path}: scan {i} has spherical but no cartesian coordinates (not supported)")
            raise RuntimeError(f"{path}: scan {i} lacks cartesianX / cartesianY / cartesianZ")
        for f in h.fields:
            if f.role in _INT_ROLES and f.kind != KIND_INT:
                raise RuntimeError(f"{path}: scan {i} field {f.name} must be an Integer field")
        scans.append(h)
    return scans


# ------------------------------------------------------------------ reading
class E57Header:
    def __init__(self, path, size, xml_offset, xml_length, scans):
        self.path = path
        self.file_size = size
        self.xml_offset = xml_offset
        self.xml_length = xml_length
        self.scans = scans


def read_bytes(path: str) -> np.ndarray:
    return np.fromfile(path, dtype=np.uint8)


def check_file_header(raw: np.ndarray, path: str):
    """(xmlPhysicalOffset, xmlLogicalLength) of a valid 48-byte header."""
    b = raw[:HEADER].tobytes()
    if b[:8] != SIGNATURE:
        raise RuntimeError(f"{path}: not an E57 file (bad signature {b[:8]!r})")
    if len(b) < HEADER:
        raise RuntimeError(f"{path}: truncated data (the file header needs {HEADER} bytes, the file has {len(b)})")
    major, minor, length, xml_off, xml_len, page = struct.unpack_from("<IIQQQQ", b, 8)
    if major != 1:
        raise RuntimeError(f"{path}: E57 major version {major} is not supported (1)")
    if page != PAGE:
        raise RuntimeError(f"{path}: page size {page} is not supported ({PAGE})")
    if length % PAGE or raw.size % PAGE:
        raise RuntimeError(f"{path}: file length {length} in the header, {raw.size} on disk: not a multiple of the "
                           f"page size {PAGE}")
    if raw.size < length:
        raise RuntimeError(f"{path}: truncated data (the header states {length} bytes, the file has {raw.size})")
    if xml_off < HEADER or xml_off % PAGE >= PAYLOAD or physical(logical(xml_off) + xml_len) > length:
        raise RuntimeError(f"{path}: truncated data (the XML section at {xml_off} + {xml_len} leaves the file)")
    return xml_off, xml_len


def raise_bad_page(path: str, bad: int, first: int):
    if bad:
        raise RuntimeError(f"{path}: CRC mismatch in page {first} ({bad} bad page{'s' if bad > 1 else ''})")


def walk_section(raw: np.ndarray, path: str, h: ScanHeader):
    """Fill the segment table of every field of scan h from its packet headers."""
    nf = len(h.fields)
    if h.section_offset % PAGE >= PAYLOAD:
        raise RuntimeError(f"{path}: scan {h.index} section offset {h.section_offset} lies in a page trailer")
    sec0 = logical(h.section_offset)
    sh = _lread(raw, path, sec0, SECTION_HEADER, f"scan {h.index} section header")
    sec_id = sh[0]
    sec_len, data_off, _index_off = struct.unpack_from("<QQQ", sh, 8)
    if sec_id != 1:
        raise RuntimeError(f"{path}: scan {h.index} section id {sec_id} is not a CompressedVector section (1)")
    end = sec0 + sec_len
    if physical(end - 1 if end else 0) >= raw.size:
        raise RuntimeError(f"{path}: truncated data (scan {h.index} section of {sec_len} bytes leaves the file)")
    pos = logical(data_off)
    segs = [[] for _ in range(nf)]
    fill = [0] * nf
    while pos < end:
        head = _lread(raw, path, pos, 4, f"scan {h.index} packet header")
        typ, plen = head[0], struct.unpack_from("<H", head, 2)[0] + 1
        if pos + plen > end:
            raise RuntimeError(f"{path}: truncated data (scan {h.index} packet at logical offset {pos} of {plen} "
                               "bytes leaves its section)")
        if typ == 1:
            cnt, = struct.unpack("<H", _lread(raw, path, pos + 4, 2, "packet header"))
            if cnt != nf:
                raise RuntimeError(f"{path}: scan {h.index} packet at logical offset {pos} has {cnt} bytestreams "
                                   f"for {nf} prototype fields")
            lens = struct.unpack(f"<{nf}H", _lread(raw, path, pos + 6, 2 * nf, "packet header"))
            at = pos + 6 + 2 * nf
            if at + sum(lens) > pos + plen:
                raise RuntimeError(f"{path}: truncated data (scan {h.index} packet at logical offset {pos}: streams "
                                   f"of {sum(lens)} bytes exceed its {plen} bytes)")
            for k, ln in enumerate(lens):
                if ln:
                    segs[k].append((fill[k], at, ln))
                    fill[k] += ln
                    at += ln
        elif typ not in (0, 2):
            raise RuntimeError(f"{path}: scan {h.index} packet type {typ} at logical offset {pos} is unknown")
        pos += plen
    for k, f in enumerate(h.fields):
        need = (h.point_count * f.bits + 7) // 8
        if fill[k] < need:
            raise RuntimeError(f"{path}: scan {h.index} stream of field {f.name} is too short for recordCount "
                               f"{h.point_count} ({fill[k]} bytes, {need} needed)")
        f.segments = np.array(segs[k], np.int64).reshape(-1, 3)


def read_header(raw: np.ndarray, path: str) -> E57Header:
    """File header, XML and every scan's segment tables (no checksum pass)."""
    xml_off, xml_len = check_file_header(raw, path)
    xml = _lread(raw, path, logical(xml_off), xml_len, "the XML section")
    scans = parse_xml(xml, path)
    for h in scans:
        walk_section(raw, path, h)
    return E57Header(path, raw.size, xml_off, xml_len, scans)


def wanted_fields(h: ScanHeader, rgb=False, intensity=False, row_column=False, invalid=True):
    """The fields of scan h a read decodes; ValueError when one asked for is missing."""
    names = ["cartesianX", "cartesianY", "cartesianZ"]
    if rgb:
        names += ["colorRed", "colorGreen", "colorBlue"]
    if intensity:
        names += ["intensity"]
    if row_column:
        names += ["rowIndex", "columnIndex"]
    out = []
    for k in names:
        f = h.field(k)
        if f is None:
            raise ValueError(f"scan {h.index} has no {k} field")
        out.append(f)
    if invalid and h.field("cartesianInvalidState") is not None:
        out.append(h.field("cartesianInvalidState"))
    return out


def _raw_values_host(raw: np.ndarray, f: E57Field, r0: int, n: int) -> np.ndarray:
    """The unsigned bit fields of records [r0, r0 + n) of f, as uint64."""
    if f.bits == 0 or n == 0:
        return np.zeros(n, np.uint64)
    bit = np.arange(r0, r0 + n, dtype=np.uint64) * np.uint64(f.bits)
    s = (bit >> np.uint64(3)).astype(np.int64)
    sh = bit & np.uint64(7)
    need = ((sh + np.uint64(f.bits + 7)) >> np.uint64(3)).astype(np.int64)
    off, logi, ln = f.segments[:, 0], f.segments[:, 1], f.segments[:, 2]
    lo = np.zeros(n, np.uint64)
    hi = np.zeros(n, np.uint64)
    for k in range((f.bits + 14) // 8):
        t = s + k
        j = np.clip(np.searchsorted(off, t, side="right") - 1, 0, len(off) - 1)
        ok = (k < need) & (t < off[j] + ln[j])
        lg = logi[j] + (t - off[j])
        p = np.where(ok, lg + 4 * (lg // PAYLOAD), 0)
        ok &= p < raw.size
        byte = np.where(ok, raw[np.minimum(p, raw.size - 1)], 0).astype(np.uint64)
        if k < 8:
            lo |= byte << np.uint64(8 * k)
        else:
            hi = byte
    v = (lo >> sh) | np.where(sh > 0, hi << ((np.uint64(64) - sh) & np.uint64(63)), np.uint64(0))
    if f.bits < 64:
        v &= np.uint64((1 << f.bits) - 1)
    return v


def _field_value_host(raw, f: E57Field, r0: int, n: int):
    v = _raw_values_host(raw, f, r0, n)
    if f.kind == KIND_F32:
        return v.astype(np.uint32).view(np.float32)
    if f.kind == KIND_F64:
        return v.view(np.float64)
    i = (v + np.uint64(f.minimum & _M64)).view(np.int64)  # wraps as the kernel's 64-bit add
    if f.kind == KIND_INT:
        return i
    return i.astype(np.float64) * np.float64(f.scale) + np.float64(f.offset)


def decode_host(raw: np.ndarray, fields, r0: int, n: int, pose=None):
    """numpy decode of records [r0, r0 + n): the values o3dx_e57_unpack
    produces.  Returns points (n,3) float64 and, for the fields given, rgb
    (n,3) uint8, intensity (n,) float32, row / col (n,) uint16, invalid (n,)
    int8 (None otherwise).  pose: pose_matrix()'s 12 values or None."""
    out = {"points": None, "rgb": None, "intensity": None, "row": None, "col": None, "invalid": None}
    val = {f.role: _field_value_host(raw, f, r0, n) for f in fields if f.role >= 0}
    with np.errstate(all="ignore"):
        if all(a in val for a in (0, 1, 2)):
            x, y, z = (val[a].astype(np.float64) for a in (0, 1, 2))
            if pose is not None:
                m = np.asarray(pose, np.float64)
                x, y, z = (m[0] * x + m[1] * y + m[2] * z + m[9], m[3] * x + m[4] * y + m[5] * z + m[10],
                           m[6] * x + m[7] * y + m[8] * z + m[11])
            out["points"] = np.stack([x, y, z], 1)
        if 3 in val:
            out["intensity"] = val[3].astype(np.float32)
        if all(a in val for a in (4, 5, 6)):
            out["rgb"] = np.stack([val[a].astype(np.uint8) for a in (4, 5, 6)], 1)
        if 7 in val:
            out["row"] = val[7].astype(np.uint16)
        if 8 in val:
            out["col"] = val[8].astype(np.uint16)
        if 9 in val:
            out["invalid"] = val[9].astype(np.int8)
    return out


def field_tables(fields):
    """(desc (k,6) int64 {role, kind, bits, minimum, first segment, segments},
    affine (k,2) float64 {scale, offset}, segments (m,3) int64) for ops.e57_unpack."""
    desc = np.zeros((len(fields), 6), np.int64)
    aff = np.zeros((len(fields), 2), np.float64)
    segs, at = [], 0
    for k, f in enumerate(fields):
        mn = f.minimum if f.minimum <= _I64_MAX else f.minimum - (1 << 64)
        desc[k] = (f.role, f.kind, f.bits, mn, at, len(f.segments))
        aff[k] = (f.scale, f.offset)
        segs.append(f.segments)
        at += len(f.segments)
    return desc, aff, (np.concatenate(segs) if segs else np.zeros((0, 3), np.int64)).reshape(-1, 3)


def decode_device(dev_raw, fields, r0: int, n: int, pose=None):
    """The same on the device (ops.e57_unpack) from the file's bytes in HBM."""
    from . import ops

    desc, aff, segs = field_tables(fields)
    return ops.e57_unpack(dev_raw, desc, aff, segs, r0, n, pose=pose)


# ------------------------------------------------------------------ writing
class ScanPlan:
    """The packet layout of one written scan: fields [(name, src kind, bits,
    minimum, maximum)], n records, R records per packet."""

    def __init__(self, fields, n: int):
        self.fields = fields
        self.n = int(n)
        nf = len(fields)
        self.head = 6 + 2 * nf
        total = sum(f[2] for f in fields)  # bits per record = bytes per 8 records
        self.R = 8 * ((MAX_PACKET - self.head) // total) if total else 8 * max((self.n + 7) // 8, 1)
        self.packets = (self.n + self.R - 1) // self.R
        self.last = self.n - (self.packets - 1) * self.R if self.packets else 0
        self.full_len = [self.R * f[2] // 8 for f in fields]
        self.last_len = [(self.last * f[2] + 7) // 8 for f in fields]
        self.full_bytes = (self.head + sum(self.full_len) + 3) // 4 * 4
        self.last_bytes = (self.head + sum(self.last_len) + 3) // 4 * 4 if self.packets else 0
        self.data_bytes = max(self.packets - 1, 0) * self.full_bytes + self.last_bytes
        self.section_bytes = SECTION_HEADER + self.data_bytes

    def packet_head(self, last: bool) -> bytes:
        lens = self.last_len if last else self.full_len
        size = self.last_bytes if last else self.full_bytes
        return struct.pack(f"<BBHH{len(lens)}H", 1, 0, size - 1, len(lens), *lens)

    def tables(self):
        """(desc (k,6) int64 {src kind, bits, minimum, offset in a full packet,
        offset in the last packet, bytes in the last packet}) for ops.e57_pack."""
        d = np.zeros((len(self.fields), 6), np.int64)
        of, ol = self.head, self.head
        for k, f in enumerate(self.fields):
            d[k] = (f[1], f[2], f[3], of, ol, self.last_len[k])
            of += self.full_len[k]
            ol += self.last_len[k]
        return d


def _bitpack(v: np.ndarray, bits: int) -> np.ndarray:
    if bits == 0 or v.size == 0:
        return np.zeros(0, np.uint8)
    if bits % 8 == 0:
        return np.ascontiguousarray(v.astype("<u8").view(np.uint8).reshape(-1, 8)[:, :bits // 8]).reshape(-1)
    b = ((v[:, None] >> np.arange(bits, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)
    return np.packbits(b.reshape(-1), bitorder="little")


def source_raw_host(src: np.ndarray, kind: int, bits: int, minimum: int) -> np.ndarray:
    """The unsigned bit field of every record of one source column."""
    if kind == SRC_F32:
        return np.ascontiguousarray(src, np.float32).view(np.uint32).astype(np.uint64)
    if kind == SRC_F64:
        return np.ascontiguousarray(src, np.float64).view(np.uint64)
    if kind == SRC_COLOUR:
        with np.errstate(all="ignore"):
            c = np.asarray(src, np.float32).astype(np.float64) * 255.0
            v = np.where(np.isnan(c), 0.0, c).astype(np.int64).astype(np.uint8).astype(np.uint64)
    else:
        v = (np.ascontiguousarray(src, np.int64).view(np.uint64) - np.uint64(minimum & _M64))
    return v & np.uint64((1 << bits) - 1) if bits < 64 else v


def pack_host(plan: ScanPlan, columns) -> np.ndarray:
    """numpy encode of one scan's packets (headers included): the bytes
    o3dx_e57_pack produces.  columns: one (n,) array per plan field."""
    out = np.zeros(plan.data_bytes, np.uint8)
    if plan.packets == 0:
        return out
    nfull = plan.packets - 1
    full = out[:nfull * plan.full_bytes].reshape(nfull, plan.full_bytes)
    last = out[nfull * plan.full_bytes:]
    full[:, :plan.head] = np.frombuffer(plan.packet_head(False), np.uint8)
    last[:plan.head] = np.frombuffer(plan.packet_head(True), np.uint8)
    desc = plan.tables()
    for k, f in enumerate(plan.fields):
        stream = _bitpack(source_raw_host(np.asarray(columns[k]).reshape(-1), f[1], f[2], f[3]), f[2])
        L = plan.full_len[k]
        full[:, desc[k, 3]:desc[k, 3] + L] = stream[:nfull * L].reshape(nfull, L)
        last[desc[k, 4]:desc[k, 4] + plan.last_len[k]] = stream[nfull * L:nfull * L + plan.last_len[k]]
    return out


def _fmt(v: float) -> str:
    return repr(float(v))


def _struct_xml(tag, items, indent):
    pad = " " * indent
    body = "".join(f"{pad}  <{k} type=\"Float\">{_fmt(v)}</{k}>\n" for k, v in items)
    return f"{pad}<{tag} type=\"Structure\">\n{body}{pad}</{tag}>\n"


def scan_xml(plan: ScanPlan, section_offset: int, name: str, guid: str, bounds, intensity_limits, rotation,
             translation, kinds) -> str:
    """The vectorChild element of one scan.  kinds: per field "single",
    "double" or (minimum, maximum)."""
    s = "    <vectorChild type=\"Structure\">\n"
    s += f"      <guid type=\"String\"><![CDATA[{guid}]]></guid>\n"
    s += f"      <name type=\"String\"><![CDATA[{escape(name)}]]></name>\n"
    if rotation is not None or translation is not None:
        q = np.array([1.0, 0, 0, 0]) if rotation is None else np.asarray(rotation, np.float64).reshape(4)
        t = np.zeros(3) if translation is None else np.asarray(translation, np.float64).reshape(3)
        s += "      <pose type=\"Structure\">\n"
        s += _struct_xml("rotation", zip("wxyz", q), 8) + _struct_xml("translation", zip("xyz", t), 8)
        s += "      </pose>\n"
    if intensity_limits is not None:
        s += _struct_xml("intensityLimits", zip(("intensityMinimum", "intensityMaximum"), intensity_limits), 6)
    if any(f[0] == "colorRed" for f in plan.fields):
        s += "      <colorLimits type=\"Structure\">\n"
        for c in ("Red", "Green", "Blue"):
            s += f"        <color{c}Minimum type=\"Integer\">0</color{c}Minimum>\n"
            s += f"        <color{c}Maximum type=\"Integer\">255</color{c}Maximum>\n"
        s += "      </colorLimits>\n"
    if bounds is not None:
        keys = ("xMinimum", "xMaximum", "yMinimum", "yMaximum", "zMinimum", "zMaximum")
        s += _struct_xml("cartesianBounds", zip(keys, bounds), 6)
    s += f"      <points type=\"CompressedVector\" fileOffset=\"{section_offset}\" recordCount=\"{plan.n}\">\n"
    s += "        <prototype type=\"Structure\">\n"
    for f, kind in zip(plan.fields, kinds):
        if isinstance(kind, str):
            s += f"          <{f[0]} type=\"Float\" precision=\"{kind}\"/>\n"
        else:
            s += f"          <{f[0]} type=\"Integer\" minimum=\"{kind[0]}\" maximum=\"{kind[1]}\"/>\n"
    s += "        </prototype>\n"
    s += "        <codecs type=\"Vector\" allowHeterogeneousChildren=\"1\"/>\n      </points>\n    </vectorChild>\n"
    return s


def file_xml(scan_parts, with_normals: bool) -> bytes:
    nor = f"\n         xmlns:nor=\"{NS_NOR}\"" if with_normals else ""
    s = "<?xml version=\"1.0\" encoding=\"UTF-8\"?>\n"
    s += f"<e57Root type=\"Structure\"\n         xmlns=\"{NS}\"{nor}>\n"
    s += "  <formatName type=\"String\"><![CDATA[ASTM E57 3D Imaging Data File]]></formatName>\n"
    s += f"  <guid type=\"String\"><![CDATA[{{{uuid.uuid4()}}}]]></guid>\n"
    s += "  <versionMajor type=\"Integer\">1</versionMajor>\n  <versionMinor type=\"Integer\">0</versionMinor>\n"
    s += f"  <e57LibraryVersion type=\"String\"><![CDATA[{LIBRARY}]]></e57LibraryVersion>\n"
    s += "  <coordinateMetadata type=\"String\"/>\n"
    s += "  <data3D type=\"Vector\" allowHeterogeneousChildren=\"1\">\n" + "".join(scan_parts) + "  </data3D>\n"
    s += "  <images2D type=\"Vector\" allowHeterogeneousChildren=\"1\"/>\n</e57Root>\n"
    return s.encode("utf-8")


def layout(plans):
    """Logical offsets of a file of these scans: (section offsets, XML offset)."""
    at, secs = HEADER, []
    for p in plans:
        secs.append(at)
        at += p.section_bytes
    return secs, at


def section_header(plan: ScanPlan, sec_logical: int) -> bytes:
    return struct.pack("<B7xQQQ", 1, plan.section_bytes, physical(sec_logical + SECTION_HEADER), 0)


def file_header(xml_logical: int, xml_len: int) -> bytes:
    total = xml_logical + xml_len
    pages = (total + PAYLOAD - 1) // PAYLOAD
    return SIGNATURE + struct.pack("<IIQQQQ", 1, 0, pages * PAGE, physical(xml_logical), xml_len, PAGE)


# ------------------------------------------------------------- the file object
class E57File:
    """What the reference's E57File (open3dpypro/E57File.py) offers its
    callers, without pye57.  The file is read and its page checksums verified
    once (on the GPU when one is visible); read / read_scan_gen decode from the
    resident bytes.  scan_headers are ScanHeader objects, not pye57 nodes.
    read applies what pye57's read_scan applies: rows with a non-zero
    cartesianInvalidState are dropped and the scan's pose transforms the
    points.  read_scan_gen yields the raw local coordinates, unfiltered, as
    the reference's raw-buffer path does, in exactly ceil(count /
    every_k_points) chunks."""

    def __init__(self, point_file, intensity=False, colors=False, row_column=False, printinfo=False):
        import torch

        self.intensity = intensity
        self.colors = colors
        self.row_column = row_column
        self.row_index = row_column
        self.column_index = row_column
        self.point_file = point_file
        if not os.path.isfile(point_file):
            raise RuntimeError(f"{point_file}: no such file")
        self._raw = read_bytes(point_file)
        self._dev = None
        check_file_header(self._raw, point_file)
        if torch.cuda.is_available():
            from . import ops

            self._dev = torch.from_numpy(self._raw).to(torch.device("cuda", torch.cuda.current_device()))
            bad, first = ops.e57_crc_pages(self._dev)
        else:
            bad, first = crc32c_pages_host(self._raw)
        raise_bad_page(point_file, bad, first)
        self.header = read_header(self._raw, point_file)
        self.scan_headers = self.header.scans
        self.scan_count = len(self.scan_headers)

        def bound(h, keys):
            return tuple(h.cartesianBounds[k] for k in keys) if h.cartesianBounds else (np.nan,) * 3

        self.scan_cartesianMinBounds = np.asarray([bound(h, ("xMinimum", "yMinimum", "zMinimum"))
                                                   for h in self.scan_headers], np.float64).reshape(-1, 3)
        self.scan_cartesianMaxBounds = np.asarray([bound(h, ("xMaximum", "yMaximum", "zMaximum"))
                                                   for h in self.scan_headers], np.float64).reshape(-1, 3)
        self.scan_headers_has_intensity = ['intensity' in h.point_fields for h in self.scan_headers]
        self.scan_headers_has_color = ['colorRed' in h.point_fields for h in self.scan_headers]
        self.scan_headers_has_row_column = [('rowIndex' in h.point_fields and 'columnIndex' in h.point_fields)
                                            for h in self.scan_headers]
        self.cartesianMinBound = self.scan_cartesianMinBounds.min(0) if self.scan_count else np.zeros(3)
        self.cartesianMaxBound = self.scan_cartesianMaxBounds.max(0) if self.scan_count else np.zeros(3)
        self.point_counts = [h.point_count for h in self.scan_headers]
        self.all_points = sum(self.point_counts)
        if printinfo:
            print('[E57File]', 'point size :', self.all_points, 'scans :', self.scan_count)
            print('[E57File]', 'each scan point size', list(zip(range(self.scan_count), self.point_counts)))
        self.datagen = self.gen()

    def close(self):
        self._raw = None
        self._dev = None

    def has_intensity(self):
        return all(self.scan_headers_has_intensity)

    def has_color(self):
        return all(self.scan_headers_has_color)

    def has_row_column(self):
        return all(self.scan_headers_has_row_column)

    # one decode: device tensors with a GPU, numpy without
    def decode(self, idx: int, r0: int, n: int, local: bool):
        """Records [r0, r0 + n) of scan idx.  local: raw coordinates, every
        row; else the pose applied and invalid rows dropped.  A dict: on the
        device points32 / points64 / wide and rgb / intensity / row / col
        tensors, on the host points and numpy columns."""
        if self._raw is None:
            raise RuntimeError(f"{self.point_file}: the E57 file is closed")
        if not 0 <= idx < self.scan_count:
            raise IndexError(f"{self.point_file}: scan {idx} of {self.scan_count}")
        h = self.scan_headers[idx]
        if r0 < 0 or n < 0 or r0 + n > h.point_count:
            raise IndexError(f"{self.point_file}: records [{r0}, {r0 + n}) of {h.point_count}")
        fields = wanted_fields(h, self.colors, self.intensity, self.row_column, invalid=not local)
        pose = pose_matrix(h.rotation, h.translation) if (h.has_pose and not local) else None
        if self._dev is None:
            d = decode_host(self._raw, fields, r0, n, pose)
            keep = None if d["invalid"] is None or not d["invalid"].any() else d["invalid"] == 0
            if keep is not None:
                d = {k: (v[keep] if v is not None else None) for k, v in d.items()}
            d["device"] = False
            return d
        t = decode_device(self._dev, fields, r0, n, pose)
        flags = int(t["flags"].item())
        if flags & FLAG_RANGE:
            raise RuntimeError(f"{self.point_file}: truncated data (scan {idx} records reach past the file)")
        wide = bool(flags & FLAG_NOT_F32)
        keep = None
        if t["invalid"] is not None and bool((t["invalid"] != 0).any().item()):
            keep = t["invalid"] == 0
        d = {"device": True}
        for k in ("points32", "points64", "rgb", "intensity", "row", "col"):
            d[k] = t[k] if (keep is None or t[k] is None) else t[k][keep]
        if keep is not None and wide:
            p = d["points64"]
            wide = not bool(((p.float().double() == p) | p.isnan()).all().item())
        d["wide"] = wide
        return d

    def _numpy(self, d):
        if d["device"]:
            cpu = lambda t: [] if t is None else t.cpu().numpy()  # noqa: E731
            xyz = d["points64"].cpu().numpy()
            inten, row, col = cpu(d["intensity"]), cpu(d["row"]), cpu(d["col"])
            if len(row):
                row, col = row.view(np.uint16), col.view(np.uint16)
            rgb = cpu(d["rgb"])
        else:
            none = lambda a: [] if a is None else a  # noqa: E731
            xyz, rgb, inten, row, col = d["points"], none(d["rgb"]), none(d["intensity"]), none(d["row"]), none(d["col"])
        self.xyz, self.rgb, self.inten, self.row_index, self.column_index = xyz, rgb, inten, row, col
        return self.xyz, self.rgb, self.inten, self.row_index, self.column_index

    def read(self, idx):
        print('[E57File@read] reading file :', self.point_file, ', idx :', idx)
        out = self._numpy(self.decode(idx, 0, self.scan_headers[idx].point_count, local=False))
        print(f'[E57File@read] reading scan : No.{idx}, points :{len(self.xyz)}, rgb :{len(self.rgb)}, '
              f'intensity :{len(self.inten)}, row_index :{len(self.row_index)}, '
              f'column_index :{len(self.column_index)}')
        return out

    def readall(self):
        parts = [self.read(i) for i in range(self.scan_count)]

        def cat(k, stack):
            a = [p[k] for p in parts if len(p[k])]
            return (np.vstack(a) if stack else np.hstack(a)) if a else []
        return cat(0, True), cat(1, True), cat(2, False), cat(3, False), cat(4, False)

    def chunks(self, idx, every_k_points):
        k = int(every_k_points)
        if k < 1:
            raise ValueError(f"every_k_points must be >= 1, got {every_k_points}")
        count = self.scan_headers[idx].point_count
        return [(r0, min(k, count - r0)) for r0 in range(0, count, k)]

    def read_scan_gen(self, idx, every_k_points=10000000):
        for data_No, (r0, m) in enumerate(self.chunks(idx, every_k_points)):
            out = self._numpy(self.decode(idx, r0, m, local=True))
            print(f'[E57File@read] reading scan : No.{idx}, ChunckNo.{data_No}, points :{len(self.xyz)}, '
                  f'rgb :{len(self.rgb)}, intensity :{len(self.inten)}, row_index :{len(self.row_index)}, '
                  f'column_index :{len(self.column_index)}')
            yield out

    def gen(self):
        for i in range(self.scan_count):
            yield self.read(i)

    def __next__(self):
        return next(self.datagen)
