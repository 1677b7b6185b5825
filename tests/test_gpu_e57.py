"""o3dx_e57_crc_pages / o3dx_e57_unpack / o3dx_e57_pack / o3dx_e57_seal and the
E57 methods on the GPU against the numpy restatement (e57_oracle.py) and the
numpy forms of e57_io.  Every comparison is exact: bit extraction, one multiply
and one add in float64, and conversions IEEE arithmetic fixes to the bit."""
import numpy as np
import pytest
import torch

import e57_oracle as EO
import open3dpypro as o3p
from open3dpypro import e57_io, ops
from test_e57_io import (BITS, FIXTURE, N_FIX, SIZES, assemble, check_packed_file, expected, geo_scan, grid_scan,
                         pack_case, write)

pytestmark = pytest.mark.gpu

KEYS = ("points", "intensity", "rgb", "row", "col")


def dirty(nbytes, dev):
    """Leave a freed block of non-zero bytes for the next allocation of this size."""
    g = torch.full((max(nbytes, 1),), 0xA5, dtype=torch.uint8, device=dev)
    del g


def to_dev(b, dev):
    return torch.from_numpy(np.frombuffer(bytes(b), np.uint8).copy()).to(dev)


def unpack(raw_dev, fields, r0, n, pose=None):
    """ops.e57_unpack with the outputs pre-dirtied, as host arrays keyed like decode_host."""
    desc, aff, segs = e57_io.field_tables(fields)
    for size in (24 * n, 12 * n, 3 * n, 4 * n, 2 * n, 2 * n, n):
        dirty(size, raw_dev.device)
    d = ops.e57_unpack(raw_dev, desc, aff, segs, r0, n, pose=pose)
    out = {"points": d["points64"].cpu().numpy(), "points32": d["points32"].cpu().numpy(),
           "flags": int(d["flags"].item())}
    for k in ("intensity", "rgb", "invalid"):
        out[k] = None if d[k] is None else d[k].cpu().numpy()
    for k in ("row", "col"):
        out[k] = None if d[k] is None else d[k].cpu().numpy().view(np.uint16)
    return out


# ---------------------------------------------------------------- checksums
@pytest.mark.parametrize("pages", [1, 63, 64, 65, 129, 700])
def test_crc_pages_equals_the_host_form(pages, dev):
    rng = np.random.default_rng(pages)
    # the last page is mostly zero padding
    paged = bytearray(EO.to_pages(rng.integers(0, 256, size=(pages - 1) * 1020 + 12, dtype=np.uint8).tobytes()))
    assert len(paged) == pages * 1024
    assert ops.e57_crc_pages(to_dev(paged, dev)) == (0, -1)
    paged[(pages - 1) * 1024 + 1019] ^= 0x01  # the last payload byte of the last page
    assert ops.e57_crc_pages(to_dev(paged, dev)) == (1, pages - 1)
    if pages > 64:
        paged[63 * 1024 + 1020] ^= 0x80  # a trailer byte
        paged[64 * 1024] ^= 0x02
        got = ops.e57_crc_pages(to_dev(paged, dev))
        bad = 2 if pages == 65 else 3  # of 65 pages, page 64 is the last one, flipped above
        assert got == (bad, 63) == e57_io.crc32c_pages_host(np.frombuffer(bytes(paged), np.uint8))


def test_crc_pages_on_the_fixture(dev):
    raw = e57_io.read_bytes(FIXTURE)
    assert ops.e57_crc_pages(torch.from_numpy(raw).to(dev)) == (0, -1)
    raw[37 * 1024 + 5] ^= 0x10
    raw[400 * 1024 + 1021] ^= 0x01
    assert ops.e57_crc_pages(torch.from_numpy(raw).to(dev)) == (2, 37)
    assert ops.e57_crc_pages(torch.empty(0, dtype=torch.uint8, device=dev)) == (0, -1)


@pytest.mark.parametrize("size", [4, 1016, 1020, 1022, 1024, 64 * 1020, 64 * 1020 + 4, 130 * 1020 - 8])
def test_seal_equals_the_oracle(size, dev):
    lg = np.random.default_rng(size).integers(1, 256, size=size, dtype=np.uint8)
    dirty((size + 1019) // 1020 * 1024, dev)
    got = ops.e57_seal(torch.from_numpy(lg).to(dev)).cpu().numpy()
    assert got.tobytes() == EO.to_pages(lg.tobytes()) == e57_io.seal_host(lg).tobytes()
    assert ops.e57_crc_pages(torch.from_numpy(got).to(dev)) == (0, -1)
    # bytes that are only 4-byte aligned take the kernel's narrow loads and stores
    shifted = torch.cat([torch.zeros(4, dtype=torch.uint8), torch.from_numpy(lg)]).to(dev)[4:]
    assert shifted.data_ptr() % 16 == 4
    assert ops.e57_seal(shifted).cpu().numpy().tobytes() == got.tobytes()


# ------------------------------------------------------------------- unpack
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("bits", BITS)
def test_unpack_equals_the_oracle(bits, n, dev):
    paged = EO.build([grid_scan(bits, n, seed=bits * 100 + n)])
    raw = np.frombuffer(paged, np.uint8)
    h = e57_io.read_header(raw, "mem").scans[0]
    want = expected(EO.read(paged)[0])
    raw_dev = to_dev(paged, dev)
    d = unpack(raw_dev, h.fields, 0, n)
    host = e57_io.decode_host(raw, h.fields, 0, n)
    for key in KEYS:
        assert d[key].dtype == want[key].dtype, key
        assert np.array_equal(d[key], want[key], equal_nan=True), key
        assert d[key].tobytes() == host[key].tobytes(), key  # the device and the numpy form: the same bits
    assert np.array_equal(d["points32"], want["points"].astype(np.float32), equal_nan=True)
    assert d["invalid"] is None and not d["flags"] & e57_io.FLAG_RANGE
    r0 = n // 3  # a chunk from the middle
    d = unpack(raw_dev, h.fields, r0, n - r0)
    for key in KEYS:
        assert np.array_equal(d[key], want[key][r0:], equal_nan=True), key
    # a subset of the fields decodes the same columns
    xyz = [f for f in h.fields if f.name.startswith("cartesian")]
    d = unpack(raw_dev, xyz, 0, n)
    assert np.array_equal(d["points"], want["points"], equal_nan=True) and d["rgb"] is None and d["row"] is None


def test_values_straddling_a_page_trailer_and_a_segment_end(dev):
    bits, n = 33, 8192
    paged = EO.build([grid_scan(bits, n, seed=7)])
    raw = np.frombuffer(paged, np.uint8)
    h = e57_io.read_header(raw, "mem").scans[0]
    f = h.field("cartesianX")
    seg = f.segments
    first, last = np.arange(n) * bits // 8, (np.arange(n) * bits + bits - 1) // 8
    sj = np.searchsorted(seg[:, 0], first, side="right") - 1
    lj = np.searchsorted(seg[:, 0], last, side="right") - 1
    across_segment = np.nonzero(sj != lj)[0]
    lg0, lg1 = seg[sj, 1] + first - seg[sj, 0], seg[lj, 1] + last - seg[lj, 0]
    across_page = np.nonzero((sj == lj) & (lg0 // 1020 != lg1 // 1020))[0]
    assert len(across_segment) >= 2 and len(across_page) >= 2
    want = expected(EO.read(paged)[0])["points"]
    d = unpack(to_dev(paged, dev), h.fields, 0, n)
    for rows in (across_segment, across_page):
        assert np.array_equal(d["points"][rows], want[rows])
    one = unpack(to_dev(paged, dev), h.fields, int(across_page[0]), 1)  # a chunk of that one record
    assert np.array_equal(one["points"], want[across_page[:1]])


def test_pose_flags_and_invalid_state(dev):
    n = 300
    inv = np.zeros(n, np.uint64)
    inv[[0, 64, 299]] = [1, 2, 1]
    pose = ([0.5, 0.5, 0.5, 0.5], [1e3, 2e3, 3.0])
    paged = EO.build([geo_scan(n, 4, pose, inv)])
    raw = np.frombuffer(paged, np.uint8)
    h = e57_io.read_header(raw, "mem").scans[0]
    o = EO.read(paged)[0]
    m = e57_io.pose_matrix(*pose)
    d = unpack(to_dev(paged, dev), h.fields, 0, n, pose=m)
    host = e57_io.decode_host(raw, h.fields, 0, n, pose=m)
    assert np.array_equal(d["points"], EO.points(o)) and d["points"].tobytes() == host["points"].tobytes()
    assert np.array_equal(d["invalid"], inv.astype(np.int8)) and d["invalid"].dtype == np.int8
    assert d["flags"] == e57_io.FLAG_NOT_F32
    d = unpack(to_dev(paged, dev), h.fields, 0, n)
    assert np.array_equal(d["points"], EO.points(o, pose=False))
    # float32 values: the flag stays clear
    fx = e57_io.read_bytes(FIXTURE)
    hf = e57_io.read_header(fx, FIXTURE).scans[0]
    d = unpack(torch.from_numpy(fx).to(dev), hf.fields, 0, N_FIX)
    assert d["flags"] == 0 and np.array_equal(d["points32"].astype(np.float64), d["points"])
    # segments that leave the file read as zero and set the range flag; nothing outside the bytes is read
    far = [e57_io.E57Field("cartesianX", e57_io.KIND_F32, 32), e57_io.E57Field("cartesianY", e57_io.KIND_F32, 32),
           e57_io.E57Field("cartesianZ", e57_io.KIND_F32, 32)]
    for f in far:
        f.segments = np.array([[0, fx.size - 40, 64]], np.int64)
    d = unpack(torch.from_numpy(fx).to(dev), far, 0, 64)
    assert d["flags"] & e57_io.FLAG_RANGE and not d["points"][16:].any()


def test_empty_and_bad_arguments(dev):
    fx = e57_io.read_bytes(FIXTURE)
    raw_dev = torch.from_numpy(fx).to(dev)
    h = e57_io.read_header(fx, FIXTURE).scans[0]
    desc, aff, segs = e57_io.field_tables(h.fields)
    d = ops.e57_unpack(raw_dev, desc, aff, segs, 0, 0)
    assert tuple(d["points64"].shape) == (0, 3) and int(d["flags"].item()) == 0
    assert len(segs) == 48
    for col, val in ((0, 10), (0, 1), (1, 7), (2, 31), (4, 40), (5, 49)):  # role, role twice, kind, bits, segments
        bad = desc.copy()
        bad[0, col] = val
        with pytest.raises(RuntimeError):
            ops.e57_unpack(raw_dev, bad, aff, segs, 0, 10)
    with pytest.raises(RuntimeError):
        ops.e57_unpack(raw_dev.cpu(), desc, aff, segs, 0, 10)
    plan, kinds, cols, _ = pack_case(13, 65)
    src = [(torch.from_numpy(c).to(dev), 1, 0) for c in cols]
    args = (plan.n, plan.R, plan.full_bytes, plan.last_bytes, plan.packet_head(False), plan.packet_head(True))
    with pytest.raises(RuntimeError):
        ops.e57_pack(plan.tables(), src, plan.n, plan.R + 1, *args[2:])
    t = plan.tables()
    t[2, 4] -= 1  # a stream overlapping the one before
    with pytest.raises(RuntimeError):
        ops.e57_pack(t, src, *args)
    with pytest.raises(RuntimeError):
        ops.e57_pack(plan.tables(), [(s[0][:10], 1, 0) for s in src], *args)
    with pytest.raises(RuntimeError):
        ops.e57_seal(torch.zeros(8, dtype=torch.uint8))


# --------------------------------------------------------------------- pack
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("bits", BITS)
def test_pack_equals_the_oracle(bits, n, dev):
    plan, kinds, cols, want = pack_case(bits, n, seed=bits + n)
    src = [(torch.from_numpy(c).to(dev), 1, 0) for c in cols]
    dirty(plan.data_bytes, dev)
    got = ops.e57_pack(plan.tables(), src, plan.n, plan.R, plan.full_bytes, plan.last_bytes, plan.packet_head(False),
                       plan.packet_head(True))
    assert got.dtype == torch.uint8 and got.numel() == plan.data_bytes
    assert got.cpu().numpy().tobytes() == e57_io.pack_host(plan, cols).tobytes()
    paged = assemble(plan, kinds, got.cpu().numpy(), lambda lg: ops.e57_seal(torch.from_numpy(lg).to(dev)).cpu()
                     .numpy().tobytes())
    check_packed_file(paged, plan, want)
    # strided sources: the columns of one (n,3)-like tensor
    if bits == 13:
        wide = [torch.stack([s[0], s[0], s[0]], 1).contiguous() for s in src]
        wide[1][:, 0], wide[1][:, 2] = 7.0, -7.0
        again = ops.e57_pack(plan.tables(), [(w, 3, 1) for w in wide], plan.n, plan.R, plan.full_bytes,
                             plan.last_bytes, plan.packet_head(False), plan.packet_head(True))
        assert torch.equal(again, got)


# ------------------------------------------------------------- the public API
def test_read_e57_fixture_on_the_device(dev):
    from open3dpypro.pcd_io import read_pcd_arrays
    import os

    fl = read_pcd_arrays(os.path.join(os.path.dirname(FIXTURE), "bunny.pcd"))
    xyz = np.stack([fl["x"], fl["y"], fl["z"]], 1).astype(np.float32)
    c = o3p.PointCloud().read_e57(FIXTURE, intensity=True)
    assert c._pts.device.type == "cuda" and c._pts.dtype == torch.float32 and c._pts_host is None
    assert c._wide is False and c._pts64 is None and c.e57._dev is not None
    assert np.array_equal(c._pts.cpu().numpy(), xyz) and np.array_equal(c.get_points(), xyz.astype(np.float64))
    assert np.array_equal(c.get_intensity().ravel(), np.asarray(fl["Intensity"], np.float32))
    raw = e57_io.read_bytes(FIXTURE)
    h = e57_io.read_header(raw, FIXTURE).scans[0]
    host = e57_io.decode_host(raw, e57_io.wanted_fields(h, intensity=True), 0, N_FIX)
    assert host["points"].tobytes() == c.get_points().tobytes()
    assert host["intensity"].tobytes() == c.get_intensity().tobytes()
    chunks = list(o3p.PointCloud().read_e57_scan_gen(FIXTURE, 0, every_k_points=3100))
    assert len(chunks) == 12 and np.array_equal(np.concatenate([k._pts.cpu().numpy() for k in chunks]), xyz)


def test_voxel_down_sample_of_a_georeferenced_e57_cloud(tmp_path, dev):
    n = 20000
    fields = []
    rng = np.random.default_rng(12)
    for a, k in enumerate(EO.ROLE_NAMES):  # a 20 m cube of millimetres at a georeferenced offset
        fields.append({"name": k, "type": "ScaledInteger", "minimum": 0, "maximum": 20000, "scale": 1e-3,
                       "offset": e57_io_offset(a), "raw": rng.integers(0, 20001, size=n).astype(np.uint64)})
    paged = EO.build([{"n": n, "fields": fields, "counts": [[n // 2] * 3, [n - n // 2] * 3]}])
    path = write(tmp_path, paged)
    pts = EO.points(EO.read(paged)[0])
    c = o3p.PointCloud().read_e57(path)
    assert c._wide is True and c._pts64 is not None and c._pts64.device.type == "cuda"
    assert np.array_equal(c.get_points(), pts)
    a = c.voxel_down_sample(0.5)
    b = o3p.PointCloud(pts).voxel_down_sample(0.5)
    assert 0 < a.size() < n and a._wide
    assert np.array_equal(a.get_points(), b.get_points())


def e57_io_offset(axis):
    from open3dpypro import synthetic

    return synthetic.LAS_OFFSET[axis]
