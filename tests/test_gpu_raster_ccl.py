"""to_2D_Img and the connected-component segmentation on the GPU, against the
reference's stored answers (tests/golden/raster_ref.npz) and the numpy
restatements of test_raster_ccl.py.  Everything is compared with array_equal:
the rasterisation is float64 arithmetic with one rounding rule, the partition
of an image into 8-connected components is algorithm-independent."""
import ctypes

import numpy as np
import pytest
import torch

import open3dpypro as o3p
from open3dpypro import _native as N
from open3dpypro import ops
from open3dpypro.PointCloudMat import PointCloudMat, ShapeType
from test_raster_ccl import (RASTER_CASES, SELECT_CASES, SIZES, ccl_ref, golden, hash_image, patterns, raster_ref,
                             select_ref)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ raster
def raster_case(name):
    g = golden()
    col = g[f"r_{name}_col"] if f"r_{name}_col" in g.files else None
    return {"pts": g[f"r_{name}_pts"], "res": float(g[f"r_{name}_res"]), "col": col, "img": g[f"r_{name}_img"],
            "ix": g[f"r_{name}_ix"], "iy": g[f"r_{name}_iy"], "T": g[f"r_{name}_T"]}


@pytest.mark.parametrize("name", RASTER_CASES)
def test_raster_fixture_cases_bit_for_bit(name, dev):
    """ops.raster2d on the stored points: pix, image and winner map, through
    the float32 entry (float32-exact values) or the float64 entry; float32-
    exact values give the same answer through both."""
    c = raster_case(name)
    wide = c["pts"].dtype == np.float64
    _, _, grey, winner, _, minx, miny = raster_ref(c["pts"], c["res"])
    dtypes = (torch.float64,) if wide else (torch.float32, torch.float64)
    for dt in dtypes:
        r = ops.raster2d(torch.as_tensor(np.array(c["pts"]), dtype=dt, device=dev), c["res"], want_winner=True)
        assert r["pix"].dtype == torch.int32 and r["img"].dtype == torch.uint8 and r["winner"].dtype == torch.int32
        pix = r["pix"].cpu().numpy()
        assert np.array_equal(pix[:, 0], c["ix"]) and np.array_equal(pix[:, 1], c["iy"])
        assert (r["h"], r["w"]) == c["img"].shape[:2] == tuple(r["img"].shape)
        assert np.array_equal(r["img"].cpu().numpy(), grey)
        if c["col"] is None:
            assert np.array_equal(grey, c["img"])
        assert np.array_equal(r["winner"].cpu().numpy(), winner)
        assert r["minx"] == minx and r["miny"] == miny
        assert ops.raster2d(torch.as_tensor(np.array(c["pts"]), dtype=dt, device=dev), c["res"])["winner"] is None


@pytest.mark.parametrize("name", RASTER_CASES)
def test_to_2D_Img_tuple(name, dev, capsys):
    c = raster_case(name)
    pts = np.array(c["pts"], np.float64)
    pc = o3p.PointCloud(pts, rgb=c["col"])
    assert pc._wide == (c["pts"].dtype == np.float64)
    out = pc.to_2D_Img(c["res"], color=c["col"] is not None)
    assert len(out) == 7
    img, minx, T, miny, invT, res, idx2img = out
    assert img.dtype == np.uint8 and np.array_equal(img, c["img"])
    assert minx == pts[:, 0].min() and miny == pts[:, 1].min() and res == c["res"]
    assert T.shape == (4, 4) and np.array_equal(T, c["T"]) and np.array_equal(invT, np.linalg.inv(c["T"]))
    assert isinstance(idx2img, np.ndarray) and idx2img.dtype == np.int64 and idx2img.shape == (len(pts), 2)
    assert np.array_equal(idx2img[:, 0], c["ix"]) and np.array_equal(idx2img[:, 1], c["iy"])
    if c["col"] is not None:  # the grey image of the same cloud; colour asked of a cloud without colours
        grey = pc.to_2D_Img(c["res"])[0]
        assert grey.ndim == 2 and np.array_equal(grey != 0, c["img"].any(2) | (grey != 0))
        capsys.readouterr()
        plain = o3p.PointCloud(pts).to_2D_Img(c["res"], color=True)[0]
        assert "has no rgb data, cannot use color!" in capsys.readouterr().out
        assert np.array_equal(plain, grey)


def test_device_only_cloud_and_degenerate_images(dev):
    c = raster_case("f32_r10")
    pc = o3p.PointCloud(torch.as_tensor(np.array(c["pts"]), device=dev))  # no host copy: the float32 points
    assert pc._pts_host is None and np.array_equal(pc.to_2D_Img(c["res"])[0], c["img"])
    line = np.zeros((40, 3))
    line[:, 1] = np.linspace(0, 3, 40)  # one pixel column
    with pytest.raises(IndexError):
        o3p.PointCloud(line).to_2D_Img(0.1)
    with pytest.raises(IndexError):
        o3p.PointCloud(line[:, [1, 0, 2]]).to_2D_Img(0.1)
    with pytest.raises(IndexError):
        ops.raster2d(torch.zeros((5, 3), device=dev), 0.1)
    with pytest.raises(RuntimeError, match="2\\^31"):
        o3p.PointCloud(np.array([[0, 0, 0], [6000.0, 6000.0, 0]])).to_2D_Img(0.1)


# ------------------------------------------------------------------- CCL
def run_ccl(im, dev):
    labels, areas, k = ops.ccl2d(torch.as_tensor(np.ascontiguousarray(im), device=dev))
    assert labels.dtype == torch.int32 and areas.dtype == torch.int64 and labels.device.type == "cuda"
    assert tuple(labels.shape) == im.shape and areas.numel() == k + 1
    return labels.cpu().numpy(), areas.cpu().numpy()


@pytest.mark.parametrize("hw", SIZES)
def test_ccl_patterns_against_the_restatement(hw, dev):
    h, w = hw
    for name, im in patterns(h, w).items():
        want, wareas = ccl_ref(im)
        labels, areas = run_ccl(im, dev)
        assert np.array_equal(areas, wareas), (name, areas[:8], wareas[:8])
        assert np.array_equal(labels, want), name
        if name == "lattice":  # the bound on the label count is reached exactly
            assert len(areas) - 1 == N.load().o3dx_ccl2d_max_labels(w, h)
        if name in ("fill41", "serpentine", "combs"):  # the same image twice: identical arrays
            l2, a2 = run_ccl(im, dev)
            assert np.array_equal(l2, labels) and np.array_equal(a2, areas), name


def test_ccl_seams_off_the_tile_grid(dev):
    """Blobs that touch only through one tile corner (64-pixel tiles), in
    both diagonal directions, and a pixel pair across each kind of seam."""
    im = np.zeros((130, 130), np.uint8)
    im[63, 63] = im[64, 64] = 1          # NW through the corner
    im[63, 128] = im[64, 127] = 1        # NE through a corner
    im[10, 63] = im[10, 64] = 1          # W across a column seam
    im[20, 63] = im[21, 64] = 1          # SW / NE across a column seam
    im[30, 64] = im[31, 63] = 1          # NW ... from the right tile's left column
    im[63, 5] = im[64, 5] = 1            # N across a row seam
    im[127, 9] = im[128, 10] = 1         # NW across the second row seam
    labels, areas = run_ccl(im, dev)
    want, wareas = ccl_ref(im)
    assert np.array_equal(labels, want) and np.array_equal(areas, wareas)
    assert len(areas) == 8 and (areas[1:] == 2).all()


# ----------------------------------------------------------- label_group
def test_label_group_order_and_counts(dev):
    h, w = 131, 67
    im = hash_image(h, w, 0.41)
    labels, areas, k = ops.ccl2d(torch.as_tensor(im, device=dev))
    n = 5000
    u = hash_image(1, 2 * n, 0.5, seed=77).ravel()  # only to draw pixel coordinates without an RNG stream
    ix = ((np.arange(n) * 2654435761 + u[:n]) % w).astype(np.int32)
    iy = ((np.arange(n) * 40503 + u[n:]) % h).astype(np.int32)
    pix = torch.as_tensor(np.stack([ix, iy], 1), device=dev)
    pl, order, counts = ops.label_group(pix, labels, k)
    assert pl.dtype == torch.int32 and order.dtype == torch.int32 and counts.dtype == torch.int64
    want_pl = labels.cpu().numpy()[iy, ix]
    assert np.array_equal(pl.cpu().numpy(), want_pl) and want_pl.max() > 0 and (want_pl == 0).any()
    assert np.array_equal(order.cpu().numpy(), np.argsort(want_pl, kind="stable"))
    assert np.array_equal(counts.cpu().numpy(), np.bincount(want_pl, minlength=k + 1))
    # k = 0: every point on the background
    zero = torch.zeros((h, w), dtype=torch.int32, device=dev)
    pl, order, counts = ops.label_group(pix, zero, 0)
    assert not pl.any() and np.array_equal(order.cpu().numpy(), np.arange(n)) and counts.cpu().numpy().tolist() == [n]


def test_label_group_rejects_a_pixel_outside_the_image(dev):
    labels = torch.zeros((8, 8), dtype=torch.int32, device=dev)
    for bad in ((8, 0), (0, 8), (-1, 3), (3, -1)):
        pix = torch.zeros((100, 2), dtype=torch.int32, device=dev)
        pix[41] = torch.tensor(bad, dtype=torch.int32)
        with pytest.raises(RuntimeError, match="outside"):
            ops.label_group(pix, labels, 0)
    L = N.load()
    pix = torch.zeros((100, 2), dtype=torch.int32, device=dev)
    pix[7, 0] = 9
    pl = torch.empty(100, dtype=torch.int32, device=dev)
    order = torch.empty(100, dtype=torch.int32, device=dev)
    cnt = torch.empty(1, dtype=torch.int64, device=dev)
    ws = torch.empty(L.o3dx_label_group_workspace_bytes(100, 0), dtype=torch.uint8, device=dev)
    rc = L.o3dx_label_group(N.ptr(pix), 100, N.ptr(labels), 8, 8, 0, N.ptr(pl), N.ptr(order), N.ptr(cnt),
                            N.ptr(ws), ws.numel(), N.stream_ptr(dev))
    assert rc == -22 and b"outside" in L.o3dx_last_error()


# ------------------------------------------------------------ end to end
def select_case(name):
    g = golden()
    offs = g[f"s_{name}_offsets"]
    return {"pts": g[f"s_{name}_pts"].astype(np.float64), "plane": g[f"s_{name}_plane"],
            "thickness": float(g[f"s_{name}_thickness"]), "res": float(g[f"s_{name}_res"]),
            "minpoints": int(g[f"s_{name}_minpoints"]), "top_n": int(g[f"s_{name}_top_n"]),
            "clouds": np.split(g[f"s_{name}_indices"], offs[1:-1]) if len(offs) > 1 else []}


@pytest.mark.parametrize("name", SELECT_CASES)
def test_segmentation_fixture_cases(name, dev):
    c = select_case(name)
    pc = o3p.PointCloud(c["pts"])
    got = pc.simple_seg_connected_components(c["plane"], c["thickness"], c["res"], c["minpoints"], c["top_n"])
    assert len(got) == len(c["clouds"])
    for q, idx in zip(got, c["clouds"]):
        assert isinstance(q, o3p.PointCloud) and np.array_equal(q.get_points(), c["pts"][idx])
    if name == "blob_over_background":  # the blob is dropped, the background stays with zero points
        assert got[0].size() == 0 and len(c["clouds"][0]) == 0
    # the processor: the same clouds' points, padded to top_n
    proc = o3p.Processors.SimpleSegConnectedComponents(plane=[float(v) for v in c["plane"]],
                                                       thickness=c["thickness"], resolution=c["res"],
                                                       minpoints=c["minpoints"], top_n=c["top_n"])
    mat = PointCloudMat(shape_type=ShapeType.XYZ).build(c["pts"])
    outs, _ = proc.validate([mat], {})
    assert len(outs) == max(c["top_n"], len(c["clouds"]))
    for m, idx in zip(outs, c["clouds"]):
        assert m.info.shape_type == ShapeType.XYZ and np.array_equal(m.data(), c["pts"][idx])
    assert all(m.data().shape == (0, 3) for m in outs[len(c["clouds"]):])


def test_by_img_on_an_edited_image(dev):
    """to_2D_Img's tuple fed back after an edit: a bridge painted between two
    blobs merges them, an erased blob's points fall to the background label."""
    c = select_case("plain")
    d = np.abs(c["pts"] @ c["plane"][:3] + c["plane"][3]) / np.linalg.norm(c["plane"][:3])
    slab = o3p.PointCloud(c["pts"][d < c["thickness"]])
    tup = slab.to_2D_Img(c["res"])
    img, idx2img = tup[0].copy(), tup[-1]
    plain = slab.simple_seg_connected_components_by_img(*tup)
    want = select_ref(tup[0], idx2img[:, 0], idx2img[:, 1])
    assert len(plain) == len(want) == 5
    for q, idx in zip(plain, want):
        assert np.array_equal(q.get_points(), slab.get_points()[idx])
    img[3, 8:13] = 255       # joins the first two rectangles
    img[10:13, 0:8] = 0      # erases the fourth
    got = slab.simple_seg_connected_components_by_img(img, *tup[1:])
    want = select_ref(img, idx2img[:, 0], idx2img[:, 1])
    assert len(got) == len(want) == 3
    for q, idx in zip(got, want):
        assert np.array_equal(q.get_points(), slab.get_points()[idx])
    assert got[0].size() == plain[0].size() + plain[1].size()
    with pytest.raises(IndexError):
        slab.simple_seg_connected_components_by_img(img[:, :-1], *tup[1:])


def test_tie_rule_empty_slab_and_attributes(dev):
    """Two patches of equal area: the higher label (the later first pixel)
    comes first.  Every attribute is carried; an empty slab gives []."""
    res = 0.1
    gx, gy = np.meshgrid(np.arange(0, 5), np.arange(0, 4))
    a = np.c_[gx.ravel() * res, gy.ravel() * res]
    b = a + [0.9, 0.0]   # 9 pixels to the right: same shape, same area
    far = np.array([[2.0, 1.5]])  # keeps the fold of the last column and row off the patches
    xy = np.concatenate([a, b, far])
    n = len(xy)
    pts = np.c_[xy, np.full(n, 0.5)]
    rng = np.random.default_rng(5)
    perm = rng.permutation(n)
    pts = pts[perm]
    nrm = rng.normal(size=(n, 3)).astype(np.float32).astype(np.float64)
    col = (rng.integers(0, 256, (n, 3)) / 255.0).astype(np.float32).astype(np.float64)
    lab = np.arange(n).reshape(-1, 1)
    pc = o3p.PointCloud(pts, rgb=col, normals=nrm, labels=lab)
    got = pc.simple_seg_connected_components([0, 0, 1, -0.5], 0.05, res, minpoints=1, top_n=100)
    assert [q.size() for q in got] == [20, 20, 1]
    first_b = np.sort(np.nonzero(np.isin(perm, np.arange(20, 40)))[0])
    first_a = np.sort(np.nonzero(np.isin(perm, np.arange(0, 20)))[0])
    for q, idx in zip(got, (first_b, first_a)):
        assert np.array_equal(q.get_points(), pts[idx])
        assert np.array_equal(q.get_normals(), nrm[idx]) and np.array_equal(q.get_colors(), col[idx])
        assert np.array_equal(q.get_labels().ravel(), idx)
    assert pc.simple_seg_connected_components([0, 0, 1, -5.0], 0.05, res) == []
    assert o3p.PointCloud().simple_seg_connected_components([0, 0, 1, 0], 0.05) == []
