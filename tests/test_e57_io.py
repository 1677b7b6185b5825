"""E57 I/O through the public API and the numpy forms (e57_io.decode_host /
pack_host / seal_host / crc32c_pages_host) against the independent numpy
restatement (e57_oracle.py) and the libE57Format-written fixture
(golden/bunny.e57).  Runs without a GPU; with one, the API assertions cover the
device path.  Every comparison is exact: the rules are bit extraction, one
multiply and one add in float64, and conversions IEEE arithmetic fixes."""
import os
import struct

import numpy as np
import pytest

import e57_oracle as EO
import open3dpypro as o3p
from open3dpypro import _native as N
from open3dpypro import e57_io, synthetic
from open3dpypro.pcd_io import read_pcd_arrays

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "bunny.e57")
N_FIX = 35947
GEO = synthetic.LAS_OFFSET
BITS = [0, 1, 7, 8, 13, 31, 32, 33, 63, 64]
SIZES = [1, 63, 64, 65, 257, 8192]
# the fixture's XML (cartesianBounds)
FIX_MIN = (-9.47000011801719666e-02, -6.19000010192394257e-02, 3.29999998211860657e-02)
FIX_MAX = (6.10000006854534149e-02, 5.88000006973743439e-02, 1.87299996614456177e-01)


# ------------------------------------------------------------------ builders
def raw_bits(n, bits, seed):
    """(n,) uint64 of `bits` random bits; zero first, all ones last."""
    if bits == 0:
        return np.zeros(n, np.uint64)
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 1 << bits, size=n, dtype=np.uint64, endpoint=False) if bits < 64 else \
        rng.integers(0, (1 << 64) - 1, size=n, dtype=np.uint64, endpoint=True)
    v[0] = 0
    v[-1] = (1 << bits) - 1
    return v


def int_field(name, bits, n, seed, typ="Integer", minimum=None, **kw):
    """An Integer / ScaledInteger field of `bits` bits with a negative minimum."""
    if minimum is None:
        minimum = -(1 << (bits - 1)) if bits else -7
    f = {"name": name, "type": typ, "minimum": minimum, "maximum": minimum + (1 << bits) - 1,
         "raw": raw_bits(n, bits, seed)}
    f.update(kw)
    return f


def split_counts(n, fields):
    """Per-packet record counts that differ between the fields, so records
    straddle packets; packets stay below 65,536 bytes."""
    total = max(sum(EO.bits_of(f) for f in fields), 1)
    per = max(1, min((n + 2) // 3, 40000 * 8 // total))
    packets = (n + per - 1) // per + 1
    rows, cum = [], [0] * len(fields)
    for j in range(1, packets + 1):
        row = []
        for k in range(len(fields)):
            c = n if j == packets else min(n, j * per + k)
            row.append(c - cum[k])
            cum[k] = c
        rows.append(row)
    return rows


def grid_scan(bits, n, seed=0):
    """One scan exercising a bit width: ScaledInteger x at a georeferenced
    offset, Integer y, Float double z, Integer intensity, colours, Integer row."""
    rng = np.random.default_rng(seed + 17)
    fields = [int_field("cartesianX", bits, n, seed + 1, "ScaledInteger", scale=1e-3, offset=GEO[0]),
              int_field("cartesianY", bits, n, seed + 2, default_limits=bits == 64),
              {"name": "cartesianZ", "type": "Float", "values": rng.normal(size=n) * 1e3},
              int_field("intensity", bits, n, seed + 3),
              int_field("colorRed", 8, n, seed + 4, minimum=0),
              int_field("colorGreen", 8, n, seed + 5, minimum=0),
              int_field("colorBlue", 8, n, seed + 6, minimum=0),
              int_field("rowIndex", bits, n, seed + 7, minimum=0 if bits < 64 else None, default_limits=bits == 64),
              int_field("columnIndex", 13, n, seed + 8, minimum=0)]
    counts = split_counts(n, fields)
    junk = {1: 0, len(counts) - 1: 2} if len(counts) > 2 else {0: 2}
    return {"n": n, "fields": fields, "counts": counts, "junk": junk}


def expected(scan_read, pose=True):
    """The columns a read returns, restated from the oracle's values."""
    v = scan_read["values"]
    out = {"points": EO.points(scan_read, pose)}
    if "intensity" in v:
        out["intensity"] = np.asarray(v["intensity"]).astype(np.float32)
    if "colorRed" in v:
        out["rgb"] = np.stack([(np.asarray(v[k], np.int64) & 0xFF).astype(np.uint8)
                               for k in ("colorRed", "colorGreen", "colorBlue")], 1)
    for key, name in (("row", "rowIndex"), ("col", "columnIndex")):
        if name in v:
            out[key] = (np.asarray(v[name], np.int64) & 0xFFFF).astype(np.uint16)
    if "cartesianInvalidState" in v:
        out["invalid"] = np.asarray(v["cartesianInvalidState"], np.int64).astype(np.int8)
    return out


def write(tmp_path, paged, name="c.e57"):
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(paged)
    return path


def reseal(paged, edit):
    """`paged` with edit(logical bytearray) applied and every trailer recomputed."""
    lg = bytearray(EO.from_pages(paged, check=False))
    edit(lg)
    return EO.to_pages(bytes(lg))


@pytest.fixture(scope="module")
def bunny_cols():
    fl = read_pcd_arrays(os.path.join(GOLDEN, "bunny.pcd"))
    return np.stack([fl["x"], fl["y"], fl["z"]], 1).astype(np.float32), np.asarray(fl["Intensity"], np.float32)


# ---------------------------------------------------------------- checksums
def test_crc32c_check_value():
    assert e57_io.crc32c(b"123456789") == 0xE3069283 == EO.crc32c(b"123456789")
    rows = np.frombuffer(b"123456789" * 3, np.uint8).reshape(3, 9)
    assert e57_io._crc_rows(rows).tolist() == [0xE3069283] * 3


def test_crc_pages_host_on_the_fixture():
    raw = e57_io.read_bytes(FIXTURE)
    assert e57_io.crc32c_pages_host(raw) == (0, -1)
    for page in (0, 1, 566):
        assert struct.unpack(">I", raw[page * 1024 + 1020:page * 1024 + 1024].tobytes())[0] == \
            EO.crc32c(raw[page * 1024:page * 1024 + 1020].tobytes())
    raw[37 * 1024 + 5] ^= 0x10
    raw[400 * 1024 + 1021] ^= 0x01
    assert e57_io.crc32c_pages_host(raw) == (2, 37)
    lg = np.frombuffer(EO.from_pages(e57_io.read_bytes(FIXTURE).tobytes()), np.uint8)
    assert e57_io.seal_host(lg).tobytes() == e57_io.read_bytes(FIXTURE).tobytes()


# ------------------------------------------------------------------ the fixture
def test_read_e57_fixture(bunny_cols):
    xyz, inten = bunny_cols
    c = o3p.PointCloud().read_e57(FIXTURE, intensity=True)
    assert isinstance(c, o3p.PointCloud) and c.size() == N_FIX
    assert c._wide is False and c._pts.dtype.is_floating_point and c._pts64 is None
    assert np.array_equal(c.get_points(), xyz.astype(np.float64))
    assert np.array_equal(c._pts.cpu().numpy(), xyz)
    assert c.get_intensity().shape == (N_FIX, 1) and c.get_intensity().dtype == np.float32
    assert np.array_equal(c.get_intensity().ravel(), inten)
    e = c.e57
    assert isinstance(e, e57_io.E57File) and c.scan_No == -1
    assert e.all_points == N_FIX and e.scan_count == 1 and e.point_counts == [N_FIX]
    assert np.array_equal(e.scan_cartesianMinBounds, [FIX_MIN]) and np.array_equal(e.scan_cartesianMaxBounds, [FIX_MAX])
    assert np.array_equal(e.cartesianMinBound, FIX_MIN) and np.array_equal(e.cartesianMaxBound, FIX_MAX)
    assert e.has_intensity() and not e.has_color() and not e.has_row_column()
    h = e.scan_headers[0]
    assert h.point_count == N_FIX and h.point_fields == ["cartesianX", "cartesianY", "cartesianZ", "intensity"]
    assert np.array_equal(h.rotation, [1, 0, 0, 0]) and np.array_equal(h.translation, [0, 0, 0])
    assert h.cartesianBounds["xMinimum"] == FIX_MIN[0] and h.section_offset == 48
    # the first stream starts at logical offset 94: floats straddle page trailers in this file
    assert h.fields[0].segments[0].tolist() == [0, 94, 12400] and len(h.fields[0].segments) == 12
    info = o3p.PointCloud().read_e57(FIXTURE, infoOnly=True)
    assert info.size() == 0 and info.e57.all_points == N_FIX
    xyz2, rgb, it, row, col = e57_io.E57File(FIXTURE, intensity=True).read(0)
    assert np.array_equal(xyz2, xyz.astype(np.float64)) and np.array_equal(it, inten)
    assert len(rgb) == 0 and len(row) == 0 and len(col) == 0
    with pytest.raises(ValueError, match="colorRed"):
        o3p.PointCloud().read_e57(FIXTURE, rgb=True)


@pytest.mark.parametrize("k", [1000, 3100, 35947, 40000])
def test_fixture_chunked_generators(k, bunny_cols):
    xyz, inten = bunny_cols
    want = -(-N_FIX // k)
    for gen in (o3p.PointCloud().read_e57_scan_gen(FIXTURE, 0, intensity=True, every_k_points=k),
                o3p.PointCloud().read_e57_gen_scan_gen(FIXTURE, intensity=True, every_k_points=k)):
        chunks = list(gen)
        assert len(chunks) == want and all(0 < c.size() <= k for c in chunks)
        assert all(c.scan_No == 0 and c.e57 is not None for c in chunks)
        assert np.array_equal(np.concatenate([c.get_points() for c in chunks]), xyz.astype(np.float64))
        assert np.array_equal(np.concatenate([c.get_intensity() for c in chunks]).ravel(), inten)
    scans = list(o3p.PointCloud().read_e57_gen(FIXTURE))
    assert len(scans) == 1 and scans[0].size() == N_FIX and scans[0].scan_No == 0
    with pytest.raises(ValueError):
        list(o3p.PointCloud().read_e57_scan_gen(FIXTURE, 0, every_k_points=0))


# ------------------------------------------------- host decode against the builder
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("bits", BITS)
def test_decode_host_equals_the_oracle(bits, n):
    paged = EO.build([grid_scan(bits, n, seed=bits * 100 + n)])
    raw = np.frombuffer(paged, np.uint8)
    assert e57_io.crc32c_pages_host(raw) == (0, -1)
    h = e57_io.read_header(raw, "mem").scans[0]
    want = expected(EO.read(paged)[0])
    d = e57_io.decode_host(raw, h.fields, 0, n)
    for key in ("points", "intensity", "rgb", "row", "col"):
        assert d[key].dtype == want[key].dtype and np.array_equal(d[key], want[key], equal_nan=True), key
    assert d["invalid"] is None
    r0 = n // 3  # a chunk from the middle
    d = e57_io.decode_host(raw, h.fields, r0, n - r0)
    for key in ("points", "intensity", "rgb", "row", "col"):
        assert np.array_equal(d[key], want[key][r0:], equal_nan=True), key


def geo_scan(n, seed, pose=None, invalid=None):
    fields = [int_field(k, 31, n, seed + a, "ScaledInteger", minimum=-(1 << 30), scale=1e-3, offset=GEO[a])
              for a, k in enumerate(EO.ROLE_NAMES)]
    fields.append({"name": "intensity", "type": "Float", "precision": "single",
                   "values": np.random.default_rng(seed).random(n).astype(np.float32)})
    if invalid is not None:
        fields.append({"name": "cartesianInvalidState", "type": "Integer", "minimum": 0, "maximum": 2,
                       "raw": np.asarray(invalid, np.uint64)})
    sc = {"n": n, "fields": fields, "counts": split_counts(n, fields)}
    if pose is not None:
        sc["pose"] = pose
    return sc


def test_scaled_integer_scan_at_georeferenced_offsets(tmp_path):
    n = 2500
    paged = EO.build([geo_scan(n, 5)])
    path = write(tmp_path, paged)
    want = expected(EO.read(paged)[0])
    c = o3p.PointCloud().read_e57(path, intensity=True)
    assert c._wide is True and c.size() == n
    assert np.array_equal(c.get_points(), want["points"])
    assert np.array_equal(c._pts.cpu().numpy(), want["points"].astype(np.float32))
    assert np.array_equal(c.get_intensity().ravel(), want["intensity"])
    assert np.abs(want["points"]).max() > 1e5  # millimetres, georeferenced-sized values


def test_two_scans_with_poses_and_invalid_rows(tmp_path):
    n0, n1 = 300, 257
    inv0 = np.zeros(n0, np.uint64)
    inv0[[0, 7, 64, 299]] = [1, 2, 1, 1]
    s = np.sqrt(0.5)
    poses = (([s, 0.0, 0.0, s], [10.0, -20.0, 0.5]), ([0.5, 0.5, 0.5, 0.5], [1e3, 2e3, 3.0]))
    paged = EO.build([geo_scan(n0, 1, poses[0], inv0), geo_scan(n1, 2, poses[1])])
    path = write(tmp_path, paged)
    o = EO.read(paged)
    keep = inv0 == 0
    w0, w1 = expected(o[0]), expected(o[1])
    assert not np.array_equal(w0["points"], EO.points(o[0], pose=False))
    c = o3p.PointCloud().read_e57(path, intensity=True)
    assert c.e57.scan_count == 2 and c.e57.point_counts == [n0, n1] and c.scan_No == -1
    assert np.array_equal(c.e57.scan_headers[1].rotation, poses[1][0])
    assert np.array_equal(c.e57.scan_headers[0].translation, poses[0][1])
    assert c.size() == keep.sum() + n1
    assert np.array_equal(c.get_points(), np.concatenate([w0["points"][keep], w1["points"]]))
    assert np.array_equal(c.get_intensity().ravel(), np.concatenate([w0["intensity"][keep], w1["intensity"]]))
    c1 = o3p.PointCloud().read_e57(path, scan_No=1)
    assert c1.scan_No == 1 and np.array_equal(c1.get_points(), w1["points"])
    per_scan = list(o3p.PointCloud().read_e57_gen(path))
    assert [p.scan_No for p in per_scan] == [0, 1]
    assert np.array_equal(per_scan[0].get_points(), w0["points"][keep])
    # the chunked generators: raw local coordinates, every row
    chunks = list(o3p.PointCloud().read_e57_gen_scan_gen(path, every_k_points=100))
    assert [p.size() for p in chunks] == [100, 100, 100, 100, 100, 57]
    assert [p.scan_No for p in chunks] == [0, 0, 0, 1, 1, 1]
    local = np.concatenate([EO.points(o[0], pose=False), EO.points(o[1], pose=False)])
    assert np.array_equal(np.concatenate([p.get_points() for p in chunks]), local)
    x, rgb, it, row, col = c.e57.readall()
    assert np.array_equal(x, c.get_points()) and len(rgb) == 0


# ------------------------------------------------------------------ the writer
def pack_case(bits, n, seed=0):
    """A ScanPlan over every source kind with two `bits`-wide integer columns
    (so the streams after them start at odd offsets): (plan, XML kinds, numpy
    columns, the raw bit fields expected back)."""
    rng = np.random.default_rng(seed + 99)
    mn = -(1 << (bits - 1)) if bits else -7
    ints = [(raw_bits(n, bits, seed + k).astype(object) + mn) for k in (1, 2)]
    ints = [np.array(v.tolist(), np.int64) for v in ints]
    f32 = rng.normal(size=n).astype(np.float32)
    f64 = rng.normal(size=n) * 1e5
    colour = rng.random(n).astype(np.float32)
    colour[0], colour[-1] = 0.0, 1.0
    S = e57_io
    fields = [("rowIndex", S.SRC_I64, bits, mn, mn + (1 << bits) - 1), ("intensity", S.SRC_F32, 32, 0, 0),
              ("columnIndex", S.SRC_I64, bits, mn, mn + (1 << bits) - 1), ("colorRed", S.SRC_COLOUR, 8, 0, 255),
              ("cartesianX", S.SRC_F64, 64, 0, 0)]
    kinds = [(mn, mn + (1 << bits) - 1), "single", (mn, mn + (1 << bits) - 1), (0, 255), "double"]
    want = {"rowIndex": raw_bits(n, bits, seed + 1), "columnIndex": raw_bits(n, bits, seed + 2),
            "intensity": f32.view(np.uint32).astype(np.uint64), "cartesianX": f64.view(np.uint64),
            "colorRed": (colour.astype(np.float64) * 255.0).astype(np.uint8).astype(np.uint64)}
    return S.ScanPlan(fields, n), kinds, [ints[0], f32, ints[1], colour, f64], want


def assemble(plan, kinds, packets, seal):
    """A file around one scan's packets, from e57_io's pieces; seal: logical uint8 -> paged bytes."""
    S = e57_io
    (sec,), xml_at = S.layout([plan])
    xml = S.file_xml([S.scan_xml(plan, S.physical(sec), "t", "{g}", None, None, None, None, kinds)], False)
    lg = np.zeros((xml_at + len(xml) + 3) // 4 * 4, np.uint8)
    lg[:48] = np.frombuffer(S.file_header(xml_at, len(xml)), np.uint8)
    lg[sec:sec + 32] = np.frombuffer(S.section_header(plan, sec), np.uint8)
    lg[sec + 32:sec + 32 + plan.data_bytes] = packets
    lg[xml_at:xml_at + len(xml)] = np.frombuffer(xml, np.uint8)
    return seal(lg)


def check_packed_file(paged, plan, want):
    sc, = EO.read(paged)  # asserts every page's trailer
    assert sc["n"] == plan.n and sc["index_offset"] == 0
    assert len(sc["packet_lengths"]) == plan.packets
    assert all(ln % 4 == 0 and ln <= 65536 for ln in sc["packet_lengths"])
    for name, raw in want.items():
        assert np.array_equal(sc["raw"][name], raw), name


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("bits", BITS)
def test_pack_host_equals_the_oracle(bits, n):
    plan, kinds, cols, want = pack_case(bits, n, seed=bits + n)
    assert plan.R % 8 == 0 and plan.full_bytes <= 65536 < plan.head + (plan.R + 8) * sum(f[2] for f in plan.fields) // 8
    packets = e57_io.pack_host(plan, cols)
    assert packets.size == plan.data_bytes
    paged = assemble(plan, kinds, packets, lambda lg: e57_io.seal_host(lg).tobytes())
    check_packed_file(paged, plan, want)
    if n == 8192:
        assert plan.packets > 1


def cloud_for_saving(n, wide, seed=3):
    rng = np.random.default_rng(seed)
    pts = rng.normal(size=(n, 3)) * 20.0
    pts = pts + np.array(GEO) if wide else pts.astype(np.float32).astype(np.float64)
    c = o3p.PointCloud(pts, rgb=rng.random((n, 3)).astype(np.float32), intensity=rng.random((n, 1)) * 300.0,
                       row_index=rng.integers(0, 1000, n), column_index=rng.integers(0, 5000, n),
                       normals=rng.normal(size=(n, 3)).astype(np.float32))
    return c, pts


@pytest.mark.parametrize("wide", [False, True])
def test_save_e57_round_trip(wide, tmp_path):
    n = 20000
    c, pts = cloud_for_saving(n, wide)
    assert c._wide is wide
    out = str(tmp_path / "s.e57")
    c.save_e57(out, name="a <scan>", rotation=[0.5, 0.5, 0.5, 0.5], translation=[1.0, 2.0, 3.0])
    with open(out, "rb") as f:
        paged = f.read()
    sc, = EO.read(paged)  # asserts every page's trailer
    assert sc["n"] == n and sc["index_offset"] == 0 and len(sc["packet_lengths"]) > 1
    assert all(ln % 4 == 0 and ln <= 65536 for ln in sc["packet_lengths"])
    names = [f["name"] for f in sc["fields"]]
    assert names == ["cartesianX", "cartesianY", "cartesianZ", "intensity", "colorRed", "colorGreen", "colorBlue",
                     "rowIndex", "columnIndex", "nor:normalX", "nor:normalY", "nor:normalZ"]
    assert sc["fields"][0]["precision"] == ("double" if wide else "single")
    assert np.array_equal(EO.points(sc, pose=False), pts)
    assert np.array_equal(sc["values"]["intensity"], np.asarray(c.get_intensity()).ravel().astype(np.float32))
    col = (c._colors.cpu().numpy().astype(np.float64) * 255.0).astype(np.uint8)
    for a, k in enumerate(("colorRed", "colorGreen", "colorBlue")):
        assert sc["fields"][4 + a]["minimum"] == 0 and sc["fields"][4 + a]["maximum"] == 255
        assert np.array_equal(sc["values"][k], col[:, a])
    assert np.array_equal(sc["values"]["rowIndex"], c.row_index)
    assert np.array_equal(sc["values"]["columnIndex"], c.column_index)
    assert sc["fields"][7]["maximum"] == c.row_index.max() and sc["fields"][8]["minimum"] == 0
    nrm = c.get_normals().astype(np.float32)
    assert np.array_equal(sc["values"]["nor:normalZ"], nrm[:, 2].astype(np.float64))
    assert sc["bounds"] == [pts[:, 0].min(), pts[:, 0].max(), pts[:, 1].min(), pts[:, 1].max(), pts[:, 2].min(),
                            pts[:, 2].max()]
    i32 = np.asarray(c.get_intensity()).ravel().astype(np.float32)
    assert sc["intensity_limits"] == [float(i32.min()), float(i32.max())]
    assert sc["pose"] == ([0.5, 0.5, 0.5, 0.5], [1.0, 2.0, 3.0])
    # our reader on our file: the pose applied, the columns back
    r = o3p.PointCloud().read_e57(out, rgb=True, intensity=True, row_column=True)
    assert r._wide is True or not wide
    assert np.array_equal(r.get_points(), EO.points(sc))
    assert np.array_equal(r.get_intensity().ravel(), i32)
    assert np.array_equal(r.row_index, c.row_index) and np.array_equal(r.column_index, c.column_index)
    cd = col.astype(np.float64)
    assert np.array_equal(r.get_colors(), ((cd - cd.min()) / (cd.max() - cd.min())).astype(np.float32).astype(np.float64))
    c.save_e57(out, normals=False)
    with open(out, "rb") as f:
        sc2, = EO.read(f.read())
    assert [f["name"] for f in sc2["fields"]] == names[:9] and sc2["pose"] is None


def test_save_pcds_e57_writes_one_scan_per_cloud(tmp_path):
    a, pa = cloud_for_saving(700, False, seed=1)
    b, pb = cloud_for_saving(65, True, seed=2)
    out = str(tmp_path / "m.e57")
    o3p.PointCloud().save_pcds_e57([a, b, o3p.PointCloud()], out)
    with open(out, "rb") as f:
        o = EO.read(f.read())
    assert [s["n"] for s in o] == [700, 65, 0]
    assert np.array_equal(EO.points(o[0]), pa) and np.array_equal(EO.points(o[1]), pb)
    assert "nor:normalX" not in [f["name"] for f in o[0]["fields"]]
    c = o3p.PointCloud().read_e57(out)
    assert c.e57.point_counts == [700, 65, 0] and np.array_equal(c.get_points(), np.concatenate([pa, pb]))


def test_e572las(tmp_path, bunny_cols):
    xyz, _ = bunny_cols
    las = str(tmp_path / "b.las")
    fr = list(o3p.PointCloud().e572las(FIXTURE, las, every_k_points=10000))
    assert fr == [10000 / N_FIX, 20000 / N_FIX, 30000 / N_FIX, 1.0]
    back = o3p.PointCloud().read_las(las)
    assert np.array_equal(back.get_points(), np.round(xyz.astype(np.float64) / 1e-4) * 1e-4 + 0.0)
    src = str(tmp_path / "c.e57")
    with open(FIXTURE, "rb") as f, open(src, "wb") as g:
        g.write(f.read())
    assert list(o3p.PointCloud().e572las(src)) == [1.0] and os.path.getsize(str(tmp_path / "c.las")) > N_FIX * 34
    with pytest.raises(NotImplementedError):
        back.save_las(las, pt_src_id=True)


# ------------------------------------------------------------------- errors
def fixture_bytes():
    with open(FIXTURE, "rb") as f:
        return f.read()


def test_errors_name_the_file_and_the_reason(tmp_path):
    good = fixture_bytes()

    def fails(paged, pattern, name):
        path = write(tmp_path, paged, name)
        with pytest.raises(RuntimeError, match=pattern) as ei:
            o3p.PointCloud().read_e57(path)
        assert path in str(ei.value)

    fails(reseal(good, lambda lg: lg.__setitem__(slice(0, 4), b"XSTM")), "bad signature", "sig.e57")
    fails(reseal(good, lambda lg: lg.__setitem__(slice(8, 12), struct.pack("<I", 2))), "major version 2", "major.e57")
    fails(reseal(good, lambda lg: lg.__setitem__(slice(40, 48), struct.pack("<Q", 2048))), "page size 2048", "page.e57")
    fails(good + b"\0" * 10, "not a multiple of the page size", "length.e57")
    fails(good[:-2048], "truncated data", "short.e57")
    flipped = bytearray(good)
    flipped[37 * 1024 + 500] ^= 0x04
    fails(bytes(flipped), "CRC mismatch in page 37", "crc.e57")
    flipped[3 * 1024 + 1022] ^= 0x80  # a trailer byte of an earlier page
    fails(bytes(flipped), r"CRC mismatch in page 3 \(2 bad pages\)", "crc2.e57")
    sc = geo_scan(100, 3)
    sc["record_count"] = 101
    fails(EO.build([sc]), "too short for recordCount 101", "count.e57")
    sph = [{"name": k, "type": "Float", "precision": "single", "values": np.zeros(4, np.float32)}
           for k in ("sphericalRange", "sphericalAzimuth", "sphericalElevation")]
    fails(EO.build([{"n": 4, "fields": sph}]), "spherical but no cartesian", "sph.e57")
    # a packet that leaves its section
    fails(reseal(good, lambda lg: lg.__setitem__(slice(56, 64), struct.pack("<Q", 575376 - 8))), "truncated data",
          "section.e57")


def test_abi_symbols_declared_and_exported():
    names = ["o3dx_e57_crc_pages", "o3dx_e57_unpack", "o3dx_e57_pack", "o3dx_e57_seal"]
    with open(N.HEADER_PATH) as f:
        header = f.read()
    lib = N.load()
    for name in names:
        assert name in N.declared_symbols() and f"int {name}(" in header and hasattr(lib, name)
    assert "E57 IO" in header and lib.o3dx_abi_version() == 7
