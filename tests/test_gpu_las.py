"""o3dx_las_unpack / o3dx_las_pack and the LAS methods on the GPU against the
numpy restatement (las_oracle.py).  Every comparison is exact: the rules are
one multiply and one add, or one subtract, one divide and one rint, in
float64, which IEEE arithmetic fixes to the bit."""
import os

import numpy as np
import pytest
import torch

import las_oracle as LO
import open3dpypro as o3p
from open3dpypro import las_io, ops, synthetic
from test_las_io import FIXTURE, attrs, cloud_X, write_case

pytestmark = pytest.mark.gpu

LIM = 2**31 - 1
GEO = synthetic.LAS_OFFSET
SC3 = (1e-3, 1e-3, 1e-3)
SIZES = [1, 63, 64, 65, 257, 8192]
LAYOUTS = [(0, 20), (2, 26), (3, 34), (3, 37), (8, 38)]  # (point format, stride)


def case_X(n, seed):
    """Random coordinates of both signs; the int32 limits in the first rows."""
    X = cloud_X(n, seed).astype(np.int64)
    X[0] = [LIM, -LIM, 0]
    if n > 1:
        X[1] = [-LIM, LIM, -1]
    return X


def dirty(nbytes, dev):
    """Leave a freed block of non-zero bytes for the next allocation of this size."""
    g = torch.full((max(nbytes, 1),), 0xA5, dtype=torch.uint8, device=dev)
    del g


def expected_records(fmt, stride, pts, scales, offsets, col=None, inten=None, cls=None):
    """The packer's rule restated: values outside int32 count and are stored as 0."""
    q = LO.quantise(pts, scales, offsets)
    over = (q < -2**31) | (q > LIM)
    X = np.where(over, 0, q)
    stats = []
    for fn, empty in ((np.min, LIM), (np.max, -2**31)):
        stats += [int(fn(q[~over[:, a], a])) if (~over[:, a]).any() else empty for a in range(3)]
    stats += [int(over.sum()), 0]
    rgb16 = None if col is None else (col.astype(np.float64) * 255.0).astype(np.uint8)
    return LO.make_records(fmt, X, stride, rgb16=rgb16, intensity=inten, labels=cls).tobytes(), stats


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("fmt,stride", LAYOUTS)
def test_unpack_equals_the_oracle(fmt, stride, n, dev):
    X = case_X(n, n + fmt)
    rgb16, inten, cls = attrs(n, n)
    has_rgb = LO.HAS_RGB[fmt]
    rec = LO.make_records(fmt, X, stride, rgb16=rgb16 if has_rgb else None, intensity=inten, labels=cls, fill=0xA5)
    raw = torch.from_numpy(np.frombuffer(rec.tobytes(), np.uint8).copy()).to(dev)
    d = ops.las_unpack(raw, n, stride, fmt, SC3, GEO, rgb=has_rgb, intensity=True, labels=True)
    want = LO.real(X, SC3, GEO)
    assert d["points64"].dtype == torch.float64 and d["points32"].dtype == torch.float32
    assert np.array_equal(d["points64"].cpu().numpy(), want)
    assert np.array_equal(d["points32"].cpu().numpy(), want.astype(np.float32))
    assert np.array_equal(d["intensity"].cpu().numpy().view(np.uint16), inten)
    assert np.array_equal(d["labels"].cpu().numpy(), cls)
    if has_rgb:
        assert np.array_equal(d["rgb"].cpu().numpy(), (rgb16 / 65536.0).astype(np.float32))
    else:
        assert d["rgb"] is None
        with pytest.raises(RuntimeError, match="no colour"):
            ops.las_unpack(raw, n, stride, fmt, SC3, GEO, rgb=True)
    assert int(d["flags"].item()) == 1  # a georeferenced millimetre grid is not float32
    plain = ops.las_unpack(raw, n, stride, fmt, SC3, GEO)
    assert plain["rgb"] is None and plain["intensity"] is None and plain["labels"] is None
    assert np.array_equal(plain["points64"].cpu().numpy(), want)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("fmt,stride", LAYOUTS)
def test_pack_equals_the_oracle(fmt, stride, n, dev):
    X = case_X(n, n + fmt)
    rgb16, inten, cls = attrs(n, n)
    has_rgb = LO.HAS_RGB[fmt]
    col = (rgb16 / 65535.0).astype(np.float32) if has_rgb else None
    pts = LO.real(X, SC3, GEO)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    for p in (pts, pts.astype(np.float32)):
        want, want_stats = expected_records(fmt, stride, p, SC3, GEO, col, inten, cls)
        dirty(n * stride, dev)
        rec, stats = ops.las_pack(up(p), stride, fmt, SC3, GEO, rgb=up(col), intensity=up(inten.view(np.int16)),
                                  labels=up(cls))
        assert rec.dtype == torch.uint8 and tuple(rec.shape) == (n, stride) and stats.dtype == torch.int64
        assert rec.cpu().numpy().tobytes() == want
        assert stats.cpu().numpy().tolist() == want_stats
        if p.dtype == np.float64:  # float64 input gives X back: nothing leaves int32
            assert want_stats[6:] == [0, 0]
            assert np.array_equal(LO.quantise(p, SC3, GEO), X)
    dirty(n * stride, dev)
    rec, _ = ops.las_pack(up(pts), stride, fmt, SC3, GEO)  # no attributes: every other byte is zero
    assert rec.cpu().numpy().tobytes() == LO.make_records(fmt, X, stride).tobytes()
    if not has_rgb:
        with pytest.raises(RuntimeError, match="no colour"):
            ops.las_pack(up(pts), stride, fmt, SC3, GEO, rgb=torch.zeros((n, 3), device=dev))


def test_empty_input(dev):
    raw = torch.empty(0, dtype=torch.uint8, device=dev)
    d = ops.las_unpack(raw, 0, 34, 3, SC3, GEO, rgb=True, intensity=True, labels=True)
    assert tuple(d["points64"].shape) == (0, 3) and tuple(d["rgb"].shape) == (0, 3) and int(d["flags"].item()) == 0
    rec, stats = ops.las_pack(torch.empty((0, 3), dtype=torch.float64, device=dev), 34, 3, SC3, GEO)
    assert tuple(rec.shape) == (0, 34)
    assert stats.cpu().numpy().tolist() == [LIM] * 3 + [-2**31] * 3 + [0, 0]


def test_bad_arguments(dev):
    raw = torch.zeros(340, dtype=torch.uint8, device=dev)
    for fmt, stride in ((11, 34), (-1, 34), (3, 33), (3, 65536)):
        with pytest.raises(RuntimeError):
            ops.las_unpack(raw, 1, stride, fmt, SC3, GEO)
    with pytest.raises(RuntimeError):
        ops.las_unpack(raw, 11, 34, 3, SC3, GEO)  # more records than bytes
    with pytest.raises(RuntimeError):
        ops.las_unpack(raw, 10, 34, 3, (0.0, 1.0, 1.0), GEO)
    x = torch.zeros((4, 3), device=dev)
    for fmt, stride in ((4, 57), (5, 63), (9, 59), (10, 67), (3, 33)):
        with pytest.raises(RuntimeError):
            ops.las_pack(x, stride, fmt, SC3, GEO)


@pytest.mark.parametrize("n", [1, 65, 257])
def test_not_float32_flag(n, dev):
    X = cloud_X(n, 7)
    rec = LO.make_records(1, X)
    raw = torch.from_numpy(np.frombuffer(rec.tobytes(), np.uint8).copy()).to(dev)
    d = ops.las_unpack(raw, n, 28, 1, (0.5,) * 3, (0.0,) * 3)  # halves of small integers: float32 values
    assert int(d["flags"].item()) == 0
    assert np.array_equal(d["points32"].cpu().numpy().astype(np.float64), d["points64"].cpu().numpy())
    d = ops.las_unpack(raw, n, 28, 1, (1e-4,) * 3, (0.0,) * 3)
    assert int(d["flags"].item()) == 1
    # one value in the last record alone sets it
    Z = np.zeros((n, 3), np.int32)
    raw0 = torch.from_numpy(np.frombuffer(LO.make_records(1, Z).tobytes(), np.uint8).copy()).to(dev)
    assert int(ops.las_unpack(raw0, n, 28, 1, (1e-4,) * 3, (0.0,) * 3)["flags"].item()) == 0
    Z[n - 1, 2] = 1
    raw1 = torch.from_numpy(np.frombuffer(LO.make_records(1, Z).tobytes(), np.uint8).copy()).to(dev)
    assert int(ops.las_unpack(raw1, n, 28, 1, (1e-4,) * 3, (0.0,) * 3)["flags"].item()) == 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pack_statistics(dtype, dev):
    n = 300
    rng = np.random.default_rng(11)
    pts = rng.uniform(-50.0, 50.0, size=(n, 3)).astype(dtype)
    pts[5, 0], pts[70, 1], pts[299, 2] = 3e5, -3e5, 2.2e5   # / 1e-4: outside int32
    pts[6, 0], pts[130, 1], pts[256, 1] = np.nan, np.inf, -np.inf
    sc, of = (1e-4,) * 3, (0.0,) * 3
    rec, stats = ops.las_pack(torch.from_numpy(pts).to(dev), 34, 3, sc, of)
    with np.errstate(all="ignore"):
        q = np.round((pts.astype(np.float64) - 0.0) / 1e-4)
    bad = ~np.isfinite(q)
    over = ~bad & ((q < -2**31) | (q > LIM))
    ok = ~(bad | over)
    want = [int(q[ok[:, a], a].min()) for a in range(3)] + [int(q[ok[:, a], a].max()) for a in range(3)] + [3, 3]
    assert stats.cpu().numpy().tolist() == want
    X = np.where(ok, q, 0.0).astype(np.int32)
    assert rec.cpu().numpy().tobytes() == LO.make_records(3, X).tobytes()
    h, hs = las_io.pack_host(pts, 3, 34, sc, of)  # the numpy form agrees
    assert h.tobytes() == rec.cpu().numpy().tobytes() and hs.tolist() == want


def test_ties_round_to_even(dev):
    k = np.arange(-40, 41, dtype=np.float64)
    x = np.concatenate([(k + 0.5) * 0.5, k + 0.25])
    pts = np.stack([x, -x, x + 0.125], 1)
    rec, _ = ops.las_pack(torch.from_numpy(pts).to(dev), 20, 0, (0.5,) * 3, (0.0,) * 3)
    assert rec.cpu().numpy().tobytes() == LO.make_records(0, np.round(pts / 0.5).astype(np.int32)).tobytes()


def test_offsets_past_2_31_bytes(dev):
    """Record offsets beyond 2^31 bytes: unpack, then pack, gives the records back."""
    stride, fmt = 67, 8
    n = 2**31 // stride + 4097
    i = torch.arange(n, dtype=torch.int64, device=dev)
    X = torch.stack([(i % 100003) - 50000, (i % 99991) * 3 - 140000, i - n // 2], 1).to(torch.int32)
    raw = torch.zeros((n, stride), dtype=torch.uint8, device=dev)
    raw[:, :12] = X.view(torch.uint8)
    raw[:, 12:14] = (i % 65521).to(torch.int16).view(-1, 1).view(torch.uint8)
    raw[:, 16] = (i % 251).to(torch.uint8)
    del i
    d = ops.las_unpack(raw.view(-1), n, stride, fmt, SC3, GEO, intensity=True, labels=True)
    tail = slice(n - 4097, n)
    want = LO.real(X[tail].cpu().numpy(), SC3, GEO)
    assert np.array_equal(d["points64"][tail].cpu().numpy(), want)
    assert np.array_equal(d["points32"][tail].cpu().numpy(), want.astype(np.float32))
    assert torch.equal(d["points64"], X.double() * 1e-3 + torch.tensor(GEO, dtype=torch.float64, device=dev))
    dirty(n * stride, dev)
    rec, stats = ops.las_pack(d["points64"], stride, fmt, SC3, GEO, intensity=d["intensity"], labels=d["labels"])
    assert torch.equal(rec, raw)
    mn, mx = X.min(0).values.cpu().tolist(), X.max(0).values.cpu().tolist()
    assert stats.cpu().numpy().tolist() == mn + mx + [0, 0]


# ------------------------------------------------------------- the public API
def host_cloud(path, rgb, intensity, labels):
    h = las_io.read_header(path)
    return las_io.decode_host(las_io.read_records(h), h, rgb, intensity, labels)


@pytest.mark.parametrize("which", ["fixture", "fmt3_extra", "fmt7_v14", "float32_grid"])
def test_read_las_equals_the_host_path(which, tmp_path):
    path = str(tmp_path / "c.las")
    rgb = which != "fixture"
    if which == "fixture":
        path = FIXTURE
    elif which == "fmt3_extra":
        write_case(path, 3, 2500, extra=3, seed=1)
    elif which == "fmt7_v14":
        write_case(path, 7, 257, seed=2, version=(1, 4), legacy_zero=True, vlr_payload=b"\x07" * 11)
    else:
        write_case(path, 2, 300, seed=3, scales=(0.25,) * 3, offsets=(1024.0, -512.0, 0.0))
    c = o3p.PointCloud().read_las(path, rgb=rgb, intensity=True, labels=True)
    d = host_cloud(path, rgb, True, True)
    ref = o3p.PointCloud(d["points"])
    assert c._pts.device.type == "cuda" and c._pts.dtype == torch.float32
    assert c._wide == ref._wide == (which != "float32_grid")
    assert (c._pts64 is not None) == c._wide
    assert np.array_equal(c.get_points(), d["points"])
    assert np.array_equal(c._pts.cpu().numpy(), d["points"].astype(np.float32))
    assert np.array_equal(c.get_intensity(), d["intensity"]) and c.get_intensity().dtype == np.uint16
    assert np.array_equal(c.get_labels(), d["labels"]) and c.get_labels().dtype == np.uint8
    if rgb:
        assert np.array_equal(c.get_colors(), d["rgb"].astype(np.float64))
    chunks = list(o3p.PointCloud().read_las_gen(path, 1000, rgb=rgb, intensity=True, labels=True))
    assert np.array_equal(np.concatenate([k.get_points() for k in chunks]), d["points"])


def test_voxel_down_sample_of_a_las_cloud():
    o = LO.read(FIXTURE)
    a = o3p.PointCloud().read_las(FIXTURE).voxel_down_sample(0.005)
    b = o3p.PointCloud(o["points"]).voxel_down_sample(0.005)
    assert 0 < a.size() < o["count"]
    assert np.array_equal(a.get_points(), b.get_points())


@pytest.mark.parametrize("float32_coords", [True, False])
def test_save_las_from_a_device_cloud(float32_coords, tmp_path, dev):
    n = 2500
    pts = LO.real(cloud_X(n, 4), SC3, GEO)
    rng = np.random.default_rng(4)
    col = rng.random((n, 3)).astype(np.float32)
    inten, lab = rng.random((n, 1)), rng.integers(0, 256, size=(n, 1))
    c = o3p.PointCloud(torch.from_numpy(pts).to(dev), rgb=torch.from_numpy(col).to(dev), intensity=inten, labels=lab)
    assert c._pts_host is None and c._wide
    out = str(tmp_path / "d.las")
    of = np.array(GEO) if not float32_coords else np.round(np.array(GEO))
    c.save_las(out, scales=SC3, offsets=of, point_format=7, float32_coords=float32_coords)
    src = pts if not float32_coords else pts.astype(np.float32)
    rec, stats = las_io.pack_host(src, 7, 36, SC3, of, rgb=col, intensity=(inten.flatten() * 255).astype(np.uint8),
                                  labels=lab.flatten().astype(np.uint8))
    ref = str(tmp_path / "h.las")
    las_io.write_file(ref, las_io.build_header(7, 36, n, SC3, of, stats), rec)
    with open(out, "rb") as f, open(ref, "rb") as g:
        a, b = f.read(), g.read()
    assert len(a) == len(b) == 227 + n * 36
    assert a[:58] == b[:58] and a[94:] == b[94:]  # all but the software string and the date
    o = LO.read(out)
    assert np.array_equal(o["X"], LO.quantise(src, SC3, of))
    # appending the same cloud doubles the records
    c.append_save_las(out)
    o2 = LO.read(out)
    assert o2["count"] == 2 * n and o2["record_bytes"][:n * 36] == o["record_bytes"]
    assert np.array_equal(o2["X"][n:], LO.quantise(pts.astype(np.float32), SC3, of))
    assert os.path.getsize(out) == 227 + 2 * n * 36
