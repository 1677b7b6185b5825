"""LAS I/O through the public API against the numpy restatement
(las_oracle.py) and the laspy-written fixture (golden/bunny_8k.las).  Runs
without a GPU (the numpy forms of the rules); with one, the same assertions
cover the device path."""
import os

import numpy as np
import pytest

import las_oracle as LO
import open3dpypro as o3p
from open3dpypro import las_io

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "bunny_8k.las")
N_FIX = 8192
SC4 = np.full(3, 1e-4)
GEO = (512345.6789, 431234.5678, 118.765)  # a georeferenced offset


def cloud_X(n, seed=0, span=200000):
    """(n,3) integer coordinates, negative values included."""
    rng = np.random.default_rng(seed)
    return rng.integers(-span, span, size=(n, 3)).astype(np.int32)


def attrs(n, seed=0):
    rng = np.random.default_rng(1000 + seed)
    return (rng.integers(0, 65536, size=(n, 3)).astype(np.uint16), rng.integers(0, 65536, size=n).astype(np.uint16),
            rng.integers(0, 256, size=n).astype(np.uint8))


def write_case(path, fmt, n, extra=0, seed=0, scales=(1e-3, 1e-3, 1e-3), offsets=GEO, **kw):
    X = cloud_X(n, seed)
    rgb16, inten, cls = attrs(n, seed)
    rec = LO.make_records(fmt, X, LO.MIN_LEN[fmt] + extra, rgb16=rgb16 if LO.HAS_RGB[fmt] else None, intensity=inten,
                          labels=cls, fill=0xA5)
    LO.write(path, fmt, rec, scales, offsets, **kw)
    return X, rgb16, inten, cls


def assert_cloud_equals_oracle(c, o, rgb):
    n = o["count"]
    assert c.size() == n
    assert np.array_equal(c.get_points().reshape(-1, 3), o["points"].reshape(-1, 3))
    if n == 0:
        return
    assert np.array_equal(c.get_intensity(), o["intensity"]) and c.get_intensity().dtype == np.uint16
    assert np.array_equal(c.get_labels(), o["labels"]) and c.get_labels().dtype == np.uint8
    assert c.get_intensity().shape == (n, 1) and c.get_labels().shape == (n, 1)
    if rgb:
        assert np.array_equal(c.get_colors(), o["rgb"].astype(np.float64))


# ------------------------------------------------------------------ the fixture
def test_read_las_fixture(bunny):
    c = o3p.PointCloud().read_las(FIXTURE)
    o = LO.read(FIXTURE)
    assert isinstance(c, o3p.PointCloud) and isinstance(c, o3p.PointCloudAdvanceIO)
    assert c.size() == N_FIX == o["count"]
    p = c.get_points()
    assert p.dtype == np.float64 and np.array_equal(p, o["points"])
    assert np.array_equal(p, np.round(bunny[:N_FIX].astype(np.float64) / 1e-4) * 1e-4 + 0.0)
    assert c._wide is True  # X * 1e-4 values are not float32 values


def test_save_las_reproduces_the_fixture(bunny, tmp_path):
    out = str(tmp_path / "bunny.las")
    o3p.PointCloud(bunny[:N_FIX]).save_las(out)
    a, b = LO.read(out), LO.read(FIXTURE)
    assert a["record_bytes"] == b["record_bytes"]
    for k in ("version", "format", "stride", "count", "legacy_count", "header_size", "data_offset", "n_vlr",
              "by_return", "system_id"):
        assert a[k] == b[k], k
    assert np.array_equal(a["scales"], b["scales"]) and np.array_equal(a["offsets"], b["offsets"])
    mins, maxs = LO.minmax(b["X"], b["scales"], b["offsets"])
    assert np.array_equal(a["mins"], mins) and np.array_equal(a["maxs"], maxs)
    assert a["tail"] == b"" and "open3dpypro" in a["software"]
    import datetime

    today = datetime.date.today()
    assert a["year"] in (today.year, today.year - 1) and 1 <= a["day"] <= 366


def test_pcd2las(tmp_path):
    import shutil

    src = str(tmp_path / "b.pcd")
    shutil.copy(os.path.join(GOLDEN, "bunny.pcd"), src)
    assert list(o3p.PointCloud().pcd2las(src)) == [0.5, 1.0]
    o = LO.read(str(tmp_path / "b.las"))
    fix = LO.read(FIXTURE)
    assert o["count"] == 35947 and o["record_bytes"][:N_FIX * 34] == fix["record_bytes"]
    # the fixture's header still holds laspy's min / max of the full file
    assert np.array_equal(o["mins"], fix["mins"]) and np.array_equal(o["maxs"], fix["maxs"])


# ------------------------------------------------------------------ round trips
@pytest.mark.parametrize("fmt", [0, 1, 2, 3, 5, 6, 7, 8])
@pytest.mark.parametrize("extra", [0, 3])
def test_read_every_format(fmt, extra, tmp_path):
    path = str(tmp_path / "c.las")
    write_case(path, fmt, 65, extra, seed=fmt)
    o = LO.read(path)
    assert o["stride"] == LO.MIN_LEN[fmt] + extra
    rgb = LO.HAS_RGB[fmt]
    c = o3p.PointCloud().read_las(path, rgb=rgb, intensity=True, labels=True)
    assert_cloud_equals_oracle(c, o, rgb)
    assert c.has_rgb() == rgb
    plain = o3p.PointCloud().read_las(path)
    assert not plain.has_rgb() and not plain.has_intensity() and not plain.has_labels()
    assert np.array_equal(plain.get_points(), o["points"])


@pytest.mark.parametrize("n", [0, 1, 65])
@pytest.mark.parametrize("layout", ["plain", "v14_legacy0", "vlr"])
def test_read_header_layouts(n, layout, tmp_path):
    path = str(tmp_path / "c.las")
    kw = {"plain": {}, "v14_legacy0": {"version": (1, 4), "legacy_zero": True},
          "vlr": {"vlr_payload": b"\x11" * 37}}[layout]
    fmt = 7 if layout == "v14_legacy0" else 3
    write_case(path, fmt, n, seed=n, **kw)
    o = LO.read(path)
    assert o["count"] == n
    if layout == "v14_legacy0":
        assert o["legacy_count"] == 0 and o["header_size"] == 375
    if layout == "vlr":
        assert o["data_offset"] == 227 + 54 + 37
    c = o3p.PointCloud().read_las(path, rgb=True, intensity=True, labels=True)
    assert_cloud_equals_oracle(c, o, True)
    if n == 0:
        assert c.is_empty()


@pytest.mark.parametrize("fmt", [0, 1, 2, 3, 6, 7, 8])
def test_save_every_writable_format(fmt, tmp_path):
    n = 65
    pts = LO.real(cloud_X(n, fmt), (1e-3,) * 3, GEO)
    rng = np.random.default_rng(fmt)
    col = rng.random((n, 3)).astype(np.float32) if LO.HAS_RGB[fmt] else None
    inten = rng.random((n, 1))
    lab = rng.integers(0, 256, size=(n, 1))
    c = o3p.PointCloud(pts, rgb=col, intensity=inten, labels=lab)
    path = str(tmp_path / "s.las")
    c.save_las(path, scales=(1e-3,) * 3, offsets=GEO, point_format=fmt, float32_coords=False)
    o = LO.read(path)
    assert (o["format"], o["stride"], o["count"], o["version"]) == (fmt, LO.MIN_LEN[fmt], n, (1, 2))
    X = LO.quantise(pts, (1e-3,) * 3, GEO)
    want = LO.make_records(fmt, X, rgb16=None if col is None else (col.astype(np.float64) * 255).astype(np.uint8),
                           intensity=(inten.flatten() * 255).astype(np.uint8), labels=lab.flatten().astype(np.uint8))
    assert o["record_bytes"] == want.tobytes()
    assert np.array_equal(o["X"], cloud_X(n, fmt))  # the quantisation undoes X * scale + offset
    mins, maxs = LO.minmax(X, (1e-3,) * 3, GEO)
    assert np.array_equal(o["mins"], mins) and np.array_equal(o["maxs"], maxs)
    back = o3p.PointCloud().read_las(path)
    assert np.array_equal(back.get_points(), pts)


def test_save_float32_coords_default(tmp_path):
    """The default casts to float32 first, as the reference; float32_coords=False does not."""
    pts = np.array([[0.123456789, 1.000049999, -2.5], [3.00005, 4.0, 5.0]])
    c = o3p.PointCloud(pts)
    a, b = str(tmp_path / "a.las"), str(tmp_path / "b.las")
    c.save_las(a)
    c.save_las(b, float32_coords=False)
    assert np.array_equal(LO.read(a)["X"], LO.quantise(pts.astype(np.float32), SC4, np.zeros(3)))
    assert np.array_equal(LO.read(b)["X"], LO.quantise(pts, SC4, np.zeros(3)))
    assert not np.array_equal(LO.read(a)["X"], LO.read(b)["X"])


def test_save_empty_cloud(tmp_path):
    path = str(tmp_path / "e.las")
    o3p.PointCloud().save_las(path)
    o = LO.read(path)
    assert o["count"] == 0 and os.path.getsize(path) == 227
    assert not o["mins"].any() and not o["maxs"].any()
    assert o3p.PointCloud().read_las(path).is_empty()


# ------------------------------------------------------------------------ chunks
@pytest.mark.parametrize("k,sizes", [(1000, [1000, 1000, 500]), (4000, [2500]), (2500, [2500])])
def test_read_las_gen(k, sizes, tmp_path, capsys):
    path = str(tmp_path / "g.las")
    write_case(path, 3, 2500, extra=3, seed=5)
    whole = o3p.PointCloud().read_las(path, rgb=True, intensity=True, labels=True)
    chunks = list(o3p.PointCloud().read_las_gen(path, k, rgb=True, intensity=True, labels=True))
    assert [c.size() for c in chunks] == sizes
    assert all(isinstance(c, o3p.PointCloud) for c in chunks)
    assert np.array_equal(np.concatenate([c.get_points() for c in chunks]), whole.get_points())
    assert np.array_equal(np.concatenate([c.get_colors() for c in chunks]), whole.get_colors())
    assert np.array_equal(np.concatenate([c.get_intensity() for c in chunks]), whole.get_intensity())
    assert np.array_equal(np.concatenate([c.get_labels() for c in chunks]), whole.get_labels())
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("[read_las_gen]")]
    assert len(lines) == len(sizes) and lines[-1] == "[read_las_gen]: read 100.0% points."


def test_read_las_gen_is_lazy(tmp_path):
    path = str(tmp_path / "g.las")
    write_case(path, 1, 10)
    g = o3p.PointCloud().read_las_gen(path, 4)
    assert next(g).size() == 4
    with pytest.raises(ValueError):
        next(o3p.PointCloud().read_las_gen(path, 0))
    assert list(o3p.PointCloud().read_las_gen(str(tmp_path / "g.las"), 4, rgb=False))[-1].size() == 2


# ------------------------------------------------------------------------ append
@pytest.mark.parametrize("layout", ["v12_fmt3", "v14_fmt7_legacy0", "v12_fmt1_extra"])
def test_append_save_las(layout, tmp_path):
    path = str(tmp_path / "a.las")
    fmt, extra, kw = {"v12_fmt3": (3, 0, {}), "v14_fmt7_legacy0": (7, 0, {"version": (1, 4), "legacy_zero": True}),
                      "v12_fmt1_extra": (1, 3, {})}[layout]
    sc = (1e-3,) * 3
    write_case(path, fmt, 65, extra, seed=2, scales=sc, offsets=GEO, **kw)
    before = LO.read(path)
    Xn = cloud_X(40, seed=9, span=400000)  # wider: moves min and max
    pts = LO.real(Xn, sc, GEO).astype(np.float32)  # float32 values: the cast is the identity
    lab = np.arange(40).reshape(-1, 1)
    o3p.PointCloud(pts, labels=lab).append_save_las(path)
    after = LO.read(path)
    assert after["count"] == 105 and after["tail"] == b""
    assert after["legacy_count"] == (0 if layout == "v14_fmt7_legacy0" else 105)
    assert after["record_bytes"][:65 * before["stride"]] == before["record_bytes"]
    Xq = LO.quantise(pts, sc, GEO)
    want = LO.make_records(fmt, Xq, before["stride"], labels=lab.flatten().astype(np.uint8))
    assert after["record_bytes"][65 * before["stride"]:] == want.tobytes()
    mins, maxs = LO.minmax(np.concatenate([before["X"], Xq]), sc, GEO)
    assert np.array_equal(after["mins"], mins) and np.array_equal(after["maxs"], maxs)
    for k in ("version", "format", "stride", "header_size", "data_offset", "by_return"):
        assert after[k] == before[k], k
    assert o3p.PointCloud().read_las(path).size() == 105


def test_append_rejections(tmp_path):
    c = o3p.PointCloud(np.zeros((2, 3)))
    with pytest.raises(AssertionError):
        c.append_save_las(str(tmp_path / "missing.las"))
    evlr = str(tmp_path / "evlr.las")
    write_case(evlr, 3, 10, tail=b"\x00" * 60)
    with pytest.raises(RuntimeError, match="EVLR"):
        c.append_save_las(evlr)
    f5 = str(tmp_path / "f5.las")
    write_case(f5, 5, 10)
    with pytest.raises(RuntimeError, match="format 5"):
        c.append_save_las(f5)
    for p in (evlr, f5):
        assert LO.read(p)["count"] == 10


# -------------------------------------------------------------------- rejections
def _bytes_of(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("case,reason", [("signature", "signature"), ("format11", "point format 11"),
                                         ("laz_bit7", "LAZ"), ("laz_bit6", "LAZ"), ("short", "shorter"),
                                         ("stride", "record length")])
def test_read_rejections(case, reason, tmp_path):
    path = str(tmp_path / f"{case}.las")
    rec = LO.make_records(3, cloud_X(10))
    if case == "signature":
        LO.write(path, 3, rec, SC4, np.zeros(3))
        b = bytearray(_bytes_of(path))
        b[0:4] = b"LASX"
        with open(path, "wb") as f:
            f.write(bytes(b))
    elif case == "format11":
        LO.write(path, 3, rec, SC4, np.zeros(3), fmt_byte=11)
    elif case == "laz_bit7":
        LO.write(path, 3, rec, SC4, np.zeros(3), fmt_byte=3 | 0x80)
    elif case == "laz_bit6":
        LO.write(path, 3, rec, SC4, np.zeros(3), fmt_byte=3 | 0x40)
    elif case == "short":
        LO.write(path, 3, rec, SC4, np.zeros(3), count=11)
    elif case == "stride":
        LO.write(path, 3, LO.make_records(2, cloud_X(10)), SC4, np.zeros(3))  # 26-byte records, format 3
    for call in (lambda: o3p.PointCloud().read_las(path), lambda: next(o3p.PointCloud().read_las_gen(path, 4))):
        with pytest.raises(RuntimeError) as e:
            call()
        assert path in str(e.value) and reason in str(e.value)


def test_rgb_on_a_format_without_colour(tmp_path):
    path = str(tmp_path / "f1.las")
    write_case(path, 1, 10)
    with pytest.raises(ValueError, match="no colour"):
        o3p.PointCloud().read_las(path, rgb=True)
    with pytest.raises(ValueError, match="no colour"):
        next(o3p.PointCloud().read_las_gen(path, 4, rgb=True))
    c = o3p.PointCloud(np.zeros((2, 3)), rgb=np.full((2, 3), 0.5))
    with pytest.raises(ValueError, match="colours"):
        c.save_las(str(tmp_path / "o.las"), point_format=1)
    assert not os.path.exists(str(tmp_path / "o.las"))


# ---------------------------------------------------------------- quantisation
def test_ties_round_to_even(tmp_path):
    k = np.arange(-6, 7, dtype=np.float64)
    x = (k + 0.5) * 0.5  # (x - 0) / 0.5 = k + 0.5: a tie
    x = np.concatenate([x, k + 0.25])  # the issue's form: values k + 0.25 at scale 0.5
    pts = np.stack([x, x, x], 1)
    path = str(tmp_path / "t.las")
    o3p.PointCloud(pts).save_las(path, scales=(0.5,) * 3)
    X = LO.read(path)["X"][:, 0]
    want = np.round(x / 0.5).astype(np.int32)
    assert np.array_equal(X, want) and (X[np.isclose(x / 0.5 % 1, 0.5)] % 2 == 0).all()
    assert np.array_equal(X[:13], [-6, -4, -4, -2, -2, 0, 0, 2, 2, 4, 4, 6, 6])


@pytest.mark.parametrize("bad,exc", [(3e5, OverflowError), (-3e5, OverflowError), (np.nan, ValueError),
                                     (np.inf, ValueError)])
def test_overflow_and_nonfinite_write_nothing(bad, exc, tmp_path):
    pts = np.zeros((70, 3))
    pts[66, 1] = bad  # 3e5 / 1e-4 = 3e9 > 2^31
    c = o3p.PointCloud(pts)
    fresh = str(tmp_path / "fresh.las")
    with pytest.raises(exc):
        c.save_las(fresh)
    assert not os.path.exists(fresh)
    kept = str(tmp_path / "kept.las")
    write_case(kept, 3, 10, scales=SC4, offsets=np.zeros(3))
    before = _bytes_of(kept)
    with pytest.raises(exc):
        c.save_las(kept)
    assert _bytes_of(kept) == before
    with pytest.raises(exc):
        c.append_save_las(kept)
    assert _bytes_of(kept) == before


def test_int32_limits_are_kept(tmp_path):
    lim = 2**31 - 1
    X = np.array([[lim, -lim, 0], [-lim, lim, lim], [-2**31, 5, -7]], np.int64)
    path = str(tmp_path / "l.las")
    o3p.PointCloud(X.astype(np.float64)).save_las(path, scales=(1.0,) * 3, float32_coords=False)
    assert np.array_equal(LO.read(path)["X"], X)
    with pytest.raises(OverflowError):
        o3p.PointCloud(X.astype(np.float64) + 1.0).save_las(path, scales=(1.0,) * 3, float32_coords=False)
    assert np.array_equal(LO.read(path)["X"], X)


# ------------------------------------------------------------------- the quirks
def test_colour_and_intensity_quirks(tmp_path):
    """The reference stores (uint8)(c * 255) in the u16 colour fields and
    (uint8)(i * 255) as intensity; read_las divides the colour by 65536."""
    col = np.array([[1.0, 0.5, 0.0], [0.999, 0.25, 0.2]], np.float32)
    inten = np.array([[1.0], [0.5]])
    c = o3p.PointCloud(np.zeros((2, 3)), rgb=col, intensity=inten)
    path = str(tmp_path / "q.las")
    c.save_las(path)
    o = LO.read(path)
    stored = np.stack([o["records"]["red"], o["records"]["green"], o["records"]["blue"]], 1)
    assert np.array_equal(stored, (col.astype(np.float64) * 255).astype(np.uint8))
    assert stored.tolist() == [[255, 127, 0], [254, 63, 51]]
    assert o["intensity"].flatten().tolist() == [255, 127]
    back = o3p.PointCloud().read_las(path, rgb=True, intensity=True)
    assert np.array_equal(back.get_colors(), stored / 65536.0)  # dimmed: at most 255 / 65536
    assert back.get_intensity().flatten().tolist() == [255, 127]


def test_labels_byte_per_format(tmp_path):
    """Formats 0-5: byte 15 whole (flag bits included); formats 6+: byte 16."""
    for fmt, off in ((1, 15), (6, 16)):
        path = str(tmp_path / f"l{fmt}.las")
        rec = LO.make_records(fmt, cloud_X(4), labels=[0xE2, 0x05, 0xFF, 0x00])
        assert rec.tobytes()[off] == 0xE2
        LO.write(path, fmt, rec, SC4, np.zeros(3))
        c = o3p.PointCloud().read_las(path, labels=True)
        assert c.get_labels().flatten().tolist() == [0xE2, 0x05, 0xFF, 0x00]


def test_not_mirrored_entries(tmp_path):
    c = o3p.PointCloud(np.zeros((2, 3)))
    with pytest.raises(NotImplementedError):
        c.save_las(str(tmp_path / "p.las"), pt_src_id=True)
    with pytest.raises(NotImplementedError):
        c.get_lasdata(None)
    assert not os.path.exists(str(tmp_path / "p.las"))


def test_host_forms_match_the_oracle():
    """las_io.decode_host / pack_host (what runs without a GPU) on their own."""
    n, fmt, stride = 257, 8, 41
    X = cloud_X(n, 3)
    rgb16, inten, cls = attrs(n, 3)
    rec = LO.make_records(fmt, X, stride, rgb16=rgb16, intensity=inten, labels=cls, fill=0x5A)
    h = las_io.LasHeader("mem", (1, 4), 375, 375, fmt, stride, n, 0, np.full(3, 1e-3), np.array(GEO), None, None, 0)
    d = las_io.decode_host(np.frombuffer(rec.tobytes(), np.uint8), h, True, True, True)
    assert np.array_equal(d["points"], LO.real(X, (1e-3,) * 3, GEO))
    assert np.array_equal(d["rgb"], (rgb16 / 65536.0).astype(np.float32))
    assert np.array_equal(d["intensity"].flatten(), inten) and np.array_equal(d["labels"].flatten(), cls)
    col = (rgb16 / 65535.0).astype(np.float32)
    out, stats = las_io.pack_host(d["points"], fmt, stride, (1e-3,) * 3, GEO, rgb=col, intensity=inten, labels=cls)
    want = LO.make_records(fmt, X, stride, rgb16=(col.astype(np.float64) * 255).astype(np.uint8), intensity=inten,
                           labels=cls)
    assert out.tobytes() == want.tobytes()
    assert stats.tolist() == X.min(0).tolist() + X.max(0).tolist() + [0, 0]
