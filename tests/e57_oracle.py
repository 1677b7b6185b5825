"""Plain numpy restatement of the E57 layout for the tests: a CRC32C, a file
builder from raw integers and a reader.  Independent of open3dpypro.e57_io
(nothing is imported from the package): bit fields are expanded to one byte
per bit (np.unpackbits / np.packbits) instead of gathered, pages are handled
as (pages, 1024) arrays, packets are walked in Python.

A scan for build():
  {"n": records, "fields": [field, ...], "counts": [[records of field 0 in
   packet 0, field 1, ...], ...] (optional; rows are data packets; a field's
   column sums to n), "junk": {packet position: packet type 0 or 2} (optional
   extra packets before that data packet), "pose": (w x y z, t) (optional),
   "bounds": 6 floats (optional)}
A field: {"name", "type": "Float" | "Integer" | "ScaledInteger", "precision"
(Float), "minimum", "maximum", "scale", "offset", "raw": (n,) uint64 bit
fields (Integer kinds) or "values": float array (Float)}.
A field's bytestream is continuous: packet k holds its bytes [floor(c_k * bits
/ 8), floor(c_{k+1} * bits / 8)) for the cumulated record counts c, the last
packet the rest, so records straddle packets.
"""
import struct
import xml.etree.ElementTree as ET

import numpy as np

NS = "http://www.astm.org/COMMIT/E57/2010-e57-v1.0"
ROLE_NAMES = ("cartesianX", "cartesianY", "cartesianZ")


def crc32c(data: bytes) -> int:
    """Bit by bit: reflected 0x82F63B78, init and final xor 0xFFFFFFFF."""
    crc = 0xFFFFFFFF
    for b in data:
        crc ^= b
        for _ in range(8):
            crc = (crc >> 1) ^ (0x82F63B78 if crc & 1 else 0)
    return crc ^ 0xFFFFFFFF


def crc32c_rows(rows: np.ndarray) -> np.ndarray:
    """The same for every row of a (k, m) uint8 array, bit by bit, all rows at once."""
    crc = np.full(len(rows), 0xFFFFFFFF, np.uint64)
    for j in range(rows.shape[1]):
        crc ^= rows[:, j].astype(np.uint64)
        for _ in range(8):
            crc = (crc >> np.uint64(1)) ^ np.where(crc & np.uint64(1), np.uint64(0x82F63B78), np.uint64(0))
    return (crc ^ np.uint64(0xFFFFFFFF)).astype(np.uint32)


def to_pages(logical: bytes) -> bytes:
    n = (len(logical) + 1019) // 1020
    pg = np.zeros((n, 1024), np.uint8)
    body = np.zeros(n * 1020, np.uint8)
    body[:len(logical)] = np.frombuffer(logical, np.uint8)
    pg[:, :1020] = body.reshape(n, 1020)
    crc = crc32c_rows(pg[:, :1020])
    for k in range(4):  # big-endian
        pg[:, 1020 + k] = (crc >> np.uint32(24 - 8 * k)) & np.uint32(0xFF)
    return pg.tobytes()


def from_pages(paged: bytes, check: bool = True) -> bytes:
    assert len(paged) % 1024 == 0
    pg = np.frombuffer(paged, np.uint8).reshape(-1, 1024)
    if check:
        crc = crc32c_rows(pg[:, :1020])
        got = sum(pg[:, 1020 + k].astype(np.uint32) << np.uint32(24 - 8 * k) for k in range(4))
        bad = np.nonzero(crc != got)[0]
        assert bad.size == 0, f"CRC mismatch in pages {bad[:8].tolist()}"
    return pg[:, :1020].tobytes()


def phys(l: int) -> int:
    return l + 4 * (l // 1020)


def bits_of(field) -> int:
    if field["type"] == "Float":
        return 32 if field.get("precision", "double") == "single" else 64
    return int(field["maximum"] - field["minimum"]).bit_length()


def field_raw(field) -> np.ndarray:
    if field["type"] == "Float":
        if bits_of(field) == 32:
            return np.asarray(field["values"], np.float32).view(np.uint32).astype(np.uint64)
        return np.asarray(field["values"], np.float64).view(np.uint64)
    return np.asarray(field["raw"], np.uint64)


def stream_bytes(raw: np.ndarray, bits: int) -> bytes:
    if bits == 0 or len(raw) == 0:
        return b""
    b = np.zeros((len(raw), bits), np.uint8)
    for k in range(bits):
        b[:, k] = (raw >> np.uint64(k)) & np.uint64(1)
    return np.packbits(b.reshape(-1), bitorder="little").tobytes()


def stream_raw(stream: bytes, bits: int, n: int) -> np.ndarray:
    if bits == 0:
        return np.zeros(n, np.uint64)
    b = np.unpackbits(np.frombuffer(stream, np.uint8), bitorder="little")[:n * bits].reshape(n, bits)
    v = np.zeros(n, np.uint64)
    for k in range(bits):
        v |= b[:, k].astype(np.uint64) << np.uint64(k)
    return v


def field_values(field, raw: np.ndarray) -> np.ndarray:
    """The decoded values: float64 for Float and ScaledInteger, int64 for Integer."""
    if field["type"] == "Float":
        if bits_of(field) == 32:
            return raw.astype(np.uint32).view(np.float32).astype(np.float64)
        return raw.view(np.float64)
    i = np.array([(int(field["minimum"]) + int(r) + (1 << 63)) % (1 << 64) - (1 << 63) for r in raw.tolist()],
                 np.int64).reshape(len(raw))
    if field["type"] == "Integer":
        return i
    return i.astype(np.float64) * np.float64(field.get("scale", 1.0)) + np.float64(field.get("offset", 0.0))


def rotation_matrix(q) -> np.ndarray:
    w, x, y, z = (float(v) for v in q)
    return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                     [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                     [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]])


def apply_pose(p: np.ndarray, q, t) -> np.ndarray:
    """x' = ((R00 x + R01 y) + R02 z) + t0, one rounded operation at a time."""
    R = rotation_matrix(q)
    out = np.empty_like(p)
    for a in range(3):
        s = R[a, 0] * p[:, 0]
        s = s + R[a, 1] * p[:, 1]
        s = s + R[a, 2] * p[:, 2]
        out[:, a] = s + float(t[a])
    return out


def _field_xml(f) -> str:
    if f["type"] == "Float":
        prec = f' precision="{f["precision"]}"' if "precision" in f else ""
        return f'<{f["name"]} type="Float"{prec}/>'
    s = f'<{f["name"]} type="{f["type"]}"'
    if not f.get("default_limits"):
        s += f' minimum="{int(f["minimum"])}" maximum="{int(f["maximum"])}"'
    if f["type"] == "ScaledInteger":
        if "scale" in f:
            s += f' scale="{float(f["scale"])!r}"'
        if "offset" in f:
            s += f' offset="{float(f["offset"])!r}"'
    return s + "/>"


def build(scans, xmlns_extra: str = "") -> bytes:
    """The paged bytes of an E57 file of these scans."""
    logical = bytearray(48)
    metas = []
    for sc in scans:
        n, fields = sc["n"], sc["fields"]
        nf = len(fields)
        counts = sc.get("counts") or [[n] * nf]
        assert all(sum(row[k] for row in counts) == n for k in range(nf))
        streams = [stream_bytes(field_raw(f), bits_of(f)) for f in fields]
        cum = [0] * nf
        at = [0] * nf
        packets = []
        for pi, row in enumerate(counts):
            pieces = []
            for k, f in enumerate(fields):
                cum[k] += row[k]
                end = len(streams[k]) if pi == len(counts) - 1 else cum[k] * bits_of(f) // 8
                pieces.append(streams[k][at[k]:end])
                at[k] = end
            body = struct.pack(f"<{nf}H", *[len(p) for p in pieces]) + b"".join(pieces)
            size = (6 + len(body) + 3) // 4 * 4
            assert size <= 65536
            pk = struct.pack("<BBHH", 1, 0, size - 1, nf) + body
            packets.append((pi, pk + b"\0" * (size - len(pk))))
        junk = sc.get("junk") or {}
        data = b""
        for pi, pk in packets:
            if pi in junk:
                typ = junk[pi]
                size = 16 if typ == 0 else 8  # skipped by their length field
                data += struct.pack("<BBH", typ, 0, size - 1) + b"\xA5" * (size - 4)
            data += pk
        sec = len(logical)
        logical += struct.pack("<B7xQQQ", 1, 32 + len(data), phys(sec + 32), 0) + data
        metas.append(phys(sec))
    xml = '<?xml version="1.0" encoding="UTF-8"?>\n'
    xml += f'<e57Root type="Structure" xmlns="{NS}"{xmlns_extra}>\n<data3D type="Vector" allowHeterogeneousChildren="1">\n'
    for sc, off in zip(scans, metas):
        xml += '<vectorChild type="Structure">\n'
        if "pose" in sc:
            q, t = sc["pose"]
            xml += '<pose type="Structure"><rotation type="Structure">'
            xml += "".join(f'<{k} type="Float">{float(v)!r}</{k}>' for k, v in zip("wxyz", q))
            xml += '</rotation><translation type="Structure">'
            xml += "".join(f'<{k} type="Float">{float(v)!r}</{k}>' for k, v in zip("xyz", t))
            xml += "</translation></pose>\n"
        if "bounds" in sc:
            keys = ("xMinimum", "xMaximum", "yMinimum", "yMaximum", "zMinimum", "zMaximum")
            xml += '<cartesianBounds type="Structure">'
            xml += "".join(f'<{k} type="Float">{float(v)!r}</{k}>' for k, v in zip(keys, sc["bounds"]))
            xml += "</cartesianBounds>\n"
        xml += f'<points type="CompressedVector" fileOffset="{off}" recordCount="{sc.get("record_count", sc["n"])}">\n'
        xml += '<prototype type="Structure">' + "".join(_field_xml(f) for f in sc["fields"]) + "</prototype>\n"
        xml += '<codecs type="Vector" allowHeterogeneousChildren="1"/></points>\n</vectorChild>\n'
    xml += '</data3D>\n<images2D type="Vector" allowHeterogeneousChildren="1"/>\n</e57Root>\n'
    xb = xml.encode()
    while len(logical) % 4:
        logical += b"\0"
    xml_at = len(logical)
    logical += xb
    pages = (len(logical) + 1019) // 1020
    logical[:48] = b"ASTM-E57" + struct.pack("<IIQQQQ", 1, 0, pages * 1024, phys(xml_at), len(xb), 1024)
    return to_pages(bytes(logical))


def _lg(p: int) -> int:
    assert p % 1024 < 1020
    return p - 4 * (p // 1024)


def read(paged: bytes, check: bool = True):
    """Every scan of a file: {"n", "fields": [{name, type, bits, minimum,
    scale, offset}], "raw": {name: uint64}, "values": {name: decoded}, "pose",
    "bounds", "packet_lengths", "index_offset"}."""
    sig, major, minor, length, xml_off, xml_len, page = struct.unpack_from("<8sIIQQQQ", paged, 0)
    assert sig == b"ASTM-E57" and major == 1 and page == 1024 and length == len(paged)
    lg = from_pages(paged, check)
    root = ET.fromstring(lg[_lg(xml_off):_lg(xml_off) + xml_len])
    q = lambda name: f"{{{NS}}}{name}"  # noqa: E731
    out = []
    for sc in root.find(q("data3D")):
        pts = sc.find(q("points"))
        n = int(pts.get("recordCount"))
        fields = []
        for el in pts.find(q("prototype")):
            name = el.tag.split("}")[1] if el.tag.startswith("{" + NS) else "nor:" + el.tag.split("}")[1]
            f = {"name": name, "type": el.get("type")}
            if f["type"] == "Float":
                f["precision"] = el.get("precision", "double")
            else:
                f["minimum"] = int(el.get("minimum", -(1 << 63)))
                f["maximum"] = int(el.get("maximum", (1 << 63) - 1))
                f["scale"] = float(el.get("scale", 1.0))
                f["offset"] = float(el.get("offset", 0.0))
            fields.append(f)
        sec = _lg(int(pts.get("fileOffset")))
        sid, sec_len, data_off, index_off = struct.unpack_from("<B7xQQQ", lg, sec)
        assert sid == 1
        pos, end = _lg(data_off), sec + sec_len
        streams = [b""] * len(fields)
        lengths = []
        while pos < end:
            typ, _, lm1 = struct.unpack_from("<BBH", lg, pos)
            if typ == 1:
                cnt, = struct.unpack_from("<H", lg, pos + 4)
                assert cnt == len(fields)
                lens = struct.unpack_from(f"<{cnt}H", lg, pos + 6)
                at = pos + 6 + 2 * cnt
                for k, ln in enumerate(lens):
                    streams[k] += lg[at:at + ln]
                    at += ln
                assert at <= pos + lm1 + 1
                lengths.append(lm1 + 1)
            pos += lm1 + 1
        assert pos == end
        raw = {f["name"]: stream_raw(streams[k], bits_of(f), n) for k, f in enumerate(fields)}
        res = {"n": n, "fields": fields, "raw": raw, "packet_lengths": lengths, "index_offset": index_off,
               "values": {f["name"]: field_values(f, raw[f["name"]]) for f in fields}, "pose": None, "bounds": None}
        pose = sc.find(q("pose"))
        if pose is not None:
            num = lambda el, d: d if el is None or not (el.text or "").strip() else float(el.text)  # noqa: E731
            r, t = pose.find(q("rotation")), pose.find(q("translation"))
            res["pose"] = ([num(r.find(q(k)), 1.0 if k == "w" else 0.0) for k in "wxyz"] if r is not None
                           else [1.0, 0, 0, 0],
                           [num(t.find(q(k)), 0.0) for k in "xyz"] if t is not None else [0.0, 0, 0])
        cb = sc.find(q("cartesianBounds"))
        if cb is not None:
            res["bounds"] = [float(cb.find(q(k)).text or 0) for k in
                             ("xMinimum", "xMaximum", "yMinimum", "yMaximum", "zMinimum", "zMaximum")]
        il = sc.find(q("intensityLimits"))
        if il is not None:
            res["intensity_limits"] = [float(il.find(q(k)).text or 0) for k in ("intensityMinimum", "intensityMaximum")]
        out.append(res)
    return out


def points(scan, pose: bool = True) -> np.ndarray:
    """(n,3) float64 of a read() scan, its pose applied when it has one."""
    p = np.stack([scan["values"][k].astype(np.float64) for k in ROLE_NAMES], 1)
    if pose and scan["pose"] is not None:
        p = apply_pose(p, *scan["pose"])
    return p
