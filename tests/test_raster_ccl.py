"""CPU: the rules behind to_2D_Img and the connected-component segmentation,
restated in numpy and pinned against tests/golden/raster_ref.npz (the
reference's own rasterisation and selection glue), the C-ABI's argument
checks, and the host side of the Python methods.  No kernel is launched here.

The restatements (raster_ref, ccl_ref, select_ref), the image patterns and the
fixture loader are shared with tests/test_gpu_raster_ccl.py.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import open3dpypro as o3p
from open3dpypro import _native as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raster_ref.npz")
RASTER_CASES = ("f32_r10", "f32_r05", "f64_offset_r07", "half_r10", "half_r05", "collide_r10", "collide_r07")
SELECT_CASES = ("plain", "blob_over_background", "minpoints", "top_n")
SYMBOLS = ("o3dx_raster2d_size", "o3dx_raster2d", "o3dx_raster2d_f64", "o3dx_ccl2d_workspace_bytes",
           "o3dx_ccl2d_max_labels", "o3dx_ccl2d", "o3dx_label_group_workspace_bytes", "o3dx_label_group")
GPU = torch.cuda.is_available()


def golden():
    return np.load(GOLDEN)


# ------------------------------------------------------------ restatements
def raster_ref(pts, resolution, colors=None):
    """to_2D_Img's rule: (ix, iy, img, winner, T, minx, miny).  ix = rint(x *
    ir + tx), the product and the sum rounded separately; the size is the
    largest index; the indices fold into [0, size - 1]; the winner of a pixel
    is its highest point index."""
    p = np.asarray(pts, np.float64)
    ir = 1 / resolution
    minx, miny = p[:, 0].min(), p[:, 1].min()
    tx, ty = ir * (-minx), ir * (-miny)
    ix = np.rint(p[:, 0] * ir + tx).astype(np.int64)
    iy = np.rint(p[:, 1] * ir + ty).astype(np.int64)
    sx, sy = int(ix.max()), int(iy.max())
    if sx < 1 or sy < 1:
        raise IndexError("empty image")
    ix = np.clip(ix, 0, sx - 1)
    iy = np.clip(iy, 0, sy - 1)
    winner = np.full((sy, sx), -1, np.int64)
    np.maximum.at(winner, (iy, ix), np.arange(len(p)))
    if colors is None:
        img = np.where(winner >= 0, 255, 0).astype(np.uint8)
    else:
        img = np.zeros((sy, sx, 3), np.uint8)
        img[winner >= 0] = (np.asarray(colors) * 255).astype(np.uint8)[winner[winner >= 0]]
    T = np.diag([ir, ir, ir, 1.0]) @ np.array([[1, 0, 0, -minx], [0, 1, 0, -miny], [0, 0, 1, 0], [0, 0, 0, 1.0]])
    return ix, iy, img, winner, T, minx, miny


def ccl_ref(img):
    """(labels int32 (h,w), areas int64 (k+1,)): 8-connected components of the
    non-zero pixels, label 0 the background, numbered by ascending row-major
    position of the first pixel.  Minimum-index trees: every round each tree's
    root takes the smallest root seen from any of its pixels' neighbours, then
    all pointers jump to their roots."""
    fg = np.asarray(img) != 0
    h, w = fg.shape
    n = h * w
    big = n
    lab = np.where(fg.ravel(), np.arange(n), big)
    idx = np.nonzero(fg.ravel())[0]
    while True:
        pad = np.full((h + 2, w + 2), big, np.int64)
        pad[1:-1, 1:-1] = lab.reshape(h, w)
        m = pad[1:-1, 1:-1].copy()
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                m = np.minimum(m, pad[dy:dy + h, dx:dx + w])
        m = m.ravel()[idx]
        before = lab[idx].copy()
        np.minimum.at(lab, lab[idx], m)
        while True:
            nxt = lab[lab[idx]]
            if np.array_equal(nxt, lab[idx]):
                break
            lab[idx] = nxt
        if np.array_equal(before, lab[idx]):
            break
    roots = np.unique(lab[idx])
    labels = np.zeros(n, np.int32)
    labels[idx] = np.searchsorted(roots, lab[idx]) + 1
    areas = np.bincount(labels, minlength=len(roots) + 1).astype(np.int64)
    return labels.reshape(h, w), areas


def ranking_ref(areas):
    """All labels by area, descending, equal areas with the higher label
    first; the first of the ranking dropped, whichever label it is."""
    return np.argsort(np.asarray(areas), kind="stable")[::-1][1:]


def select_ref(img, ix, iy, minpoints=0, top_n=None):
    """The index lists simple_seg_connected_components returns (by_img's with
    top_n=None, minpoints=0)."""
    labels, areas = ccl_ref(img)
    pl = labels[iy, ix]
    rank = ranking_ref(areas)
    if top_n is not None:
        rank = rank[:top_n]
    out = [np.nonzero(pl == l)[0] for l in rank]
    return [o for o in out if len(o) >= minpoints]


# ------------------------------------------------------------ image patterns
def _fmix32(h):
    h = h.copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def hash_image(h, w, fill, seed=0x9E3779B9):
    """uint8 image, 255 with probability `fill`, from the integer hash of
    tests/test_dbscan.py on the pixel index (no RNG stream)."""
    with np.errstate(over="ignore"):
        k = (np.arange(h * w, dtype=np.uint64) + np.uint64(seed)).astype(np.uint32)
        u = _fmix32(_fmix32(k) + np.uint32(seed))
    return np.where(u.astype(np.float64) / 4294967296.0 < fill, 255, 0).astype(np.uint8).reshape(h, w)


def serpentine(h, w):
    """A 1-pixel path through every even row, joined at alternating ends: one
    component crossing every seam."""
    im = np.zeros((h, w), np.uint8)
    im[0::2] = 255
    for k, y in enumerate(range(1, h, 2)):
        im[y, w - 1 if k % 2 == 0 else 0] = 255
    return im


def spiral(h, w):
    """A square spiral: 1-pixel rings two apart, each opened below its top-left
    corner and joined there to the next ring inwards: one component."""
    im = np.zeros((h, w), np.uint8)
    o = 0
    while h - 1 - o >= o and w - 1 - o >= o:
        t, l, b, r = o, o, h - 1 - o, w - 1 - o
        im[t, l:r + 1] = im[b, l:r + 1] = 255
        im[t:b + 1, l] = im[t:b + 1, r] = 255
        if b - t < 4 or r - l < 4:
            break
        im[t + 1, l] = 0
        im[t + 2, l + 1] = 255
        o += 2
    return im


def combs(h, w):
    """Vertical teeth every other column joined only along the bottom row, in
    two combs split by an empty column band; the left comb's first tooth
    starts lower, so its first pixel is not at its bounding box's corner."""
    im = np.zeros((h, w), np.uint8)
    if h < 2 or w < 2:
        return im
    im[:, 0::2] = 255
    im[h - 1, :] = 255
    if w >= 8:
        mid = w // 2
        im[:, mid - 1:mid + 2] = 0
    im[0:min(3, h - 1), 0] = 0
    return im


def patterns(h, w):
    """name -> image, for one size."""
    yy, xx = np.mgrid[0:h, 0:w]
    out = {
        "zero": np.zeros((h, w), np.uint8),
        "full": np.full((h, w), 255, np.uint8),
        "fill20": hash_image(h, w, 0.2),
        "fill41": hash_image(h, w, 0.41),
        "fill60": hash_image(h, w, 0.6),
        "checker": np.where((yy + xx) % 2 == 0, 1, 0).astype(np.uint8),
        "anti_diag": np.where((yy + xx) % 3 == 0, 255, 0).astype(np.uint8),
        "main_diag": np.where((yy - xx) % 3 == 0, 255, 0).astype(np.uint8),
        "lattice": np.where((yy % 2 == 0) & (xx % 2 == 0), 7, 0).astype(np.uint8),
        "serpentine": serpentine(h, w),
        "spiral": spiral(h, w),
        "combs": combs(h, w),
    }
    return out


SIZES = ((1, 1), (2, 2), (1, 300), (300, 1), (67, 131), (129, 257), (515, 513))  # (h, w)


# ----------------------------------------------------------------- the tests
def test_symbols_are_declared_and_exported():
    lib = N.load()
    for s in SYMBOLS:
        assert s in N.declared_symbols() and hasattr(lib, s), s
    for m in ("to_2D_Img", "simple_seg_connected_components", "simple_seg_connected_components_by_img"):
        assert hasattr(o3p.PointCloud, m), m


@pytest.mark.parametrize("name", RASTER_CASES)
def test_raster_ref_matches_the_reference(name):
    g = golden()
    pts, res = g[f"r_{name}_pts"], float(g[f"r_{name}_res"])
    col = g[f"r_{name}_col"] if f"r_{name}_col" in g.files else None
    ix, iy, img, winner, T, minx, miny = raster_ref(pts, res, col)
    assert np.array_equal(ix, g[f"r_{name}_ix"]) and np.array_equal(iy, g[f"r_{name}_iy"])
    assert img.shape == g[f"r_{name}_img"].shape and np.array_equal(img, g[f"r_{name}_img"])
    assert np.array_equal(T, g[f"r_{name}_T"])


def test_half_pixel_case_exercises_half_to_even():
    """The fixture's half-pixel case holds points whose x * ir + tx is exactly
    k + 0.5 for even and odd k: floor(v + 0.5) would differ from rint."""
    g = golden()
    pts, res = g["r_half_r10_pts"], float(g["r_half_r10_res"])
    ir = 1 / res
    v = pts[:, 0] * ir + ir * (-pts[:, 0].min())
    half = v - np.floor(v) == 0.5
    k = np.floor(v[half]).astype(np.int64)
    assert (k % 2 == 0).any() and (k % 2 == 1).any()
    assert not np.array_equal(np.floor(v + 0.5), np.rint(v))


@pytest.mark.parametrize("name", RASTER_CASES)
def test_raster2d_size_matches_the_reference_shapes(name):
    g = golden()
    pts, res = g[f"r_{name}_pts"], float(g[f"r_{name}_res"])
    w, h = o3p.ops.raster2d_size(res, pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].max(), pts[:, 1].max())
    assert (h, w) == g[f"r_{name}_img"].shape[:2]


def test_raster2d_size_random_clouds():
    """The size from the bounds equals the largest index of the cloud
    (monotone maps): float32-exact and float64 values, offsets, resolutions."""
    rng = np.random.default_rng(12)
    for trial in range(60):
        res = float(rng.choice([0.005, 0.05, 0.07, 0.1, 0.33, 1.0]))
        off = rng.choice([0.0, 4.5e5, 6e6]) * rng.uniform(-1, 1, 3)
        p = off + rng.uniform(0, 1, (200, 3)) * rng.choice([1.0, 30.0])
        if trial % 2:
            p = p.astype(np.float32).astype(np.float64)
        ir = 1 / res
        ix = np.rint(p[:, 0] * ir + ir * (-p[:, 0].min())).astype(np.int64)
        iy = np.rint(p[:, 1] * ir + ir * (-p[:, 1].min())).astype(np.int64)
        assert o3p.ops.raster2d_size(res, p[:, 0].min(), p[:, 1].min(), p[:, 0].max(), p[:, 1].max()) == \
            (int(ix.max()), int(iy.max()))


@pytest.mark.parametrize("name", SELECT_CASES)
def test_select_ref_matches_the_reference(name):
    g = golden()
    pts = g[f"s_{name}_pts"]
    plane, thick, res = g[f"s_{name}_plane"], float(g[f"s_{name}_thickness"]), float(g[f"s_{name}_res"])
    minpoints, top_n = int(g[f"s_{name}_minpoints"]), int(g[f"s_{name}_top_n"])
    d = np.abs(pts @ plane[:3].reshape(3, 1) + plane[3]) / (plane[:3] ** 2).sum() ** 0.5
    slab = np.nonzero(d.ravel() < thick)[0]
    ix, iy, img, *_ = raster_ref(pts[slab], res)
    got = [slab[o] for o in select_ref(img, ix, iy, minpoints, top_n)]
    offs = g[f"s_{name}_offsets"]
    exp = np.split(g[f"s_{name}_indices"], offs[1:-1])
    assert len(got) == len(exp) == len(offs) - 1
    for a, b in zip(got, exp):
        assert np.array_equal(a, b)


def test_ccl_ref_small_cases():
    im = np.array([[0, 9, 0, 0, 1],
                   [0, 0, 0, 1, 0],
                   [1, 0, 0, 0, 0],
                   [1, 1, 0, 0, 2]], np.uint8)
    lab, areas = ccl_ref(im)
    assert np.array_equal(lab, [[0, 1, 0, 0, 2], [0, 0, 0, 2, 0], [3, 0, 0, 0, 0], [3, 3, 0, 0, 4]])
    assert np.array_equal(areas, [13, 1, 2, 3, 1])
    lab, areas = ccl_ref(np.zeros((3, 4), np.uint8))
    assert not lab.any() and np.array_equal(areas, [12])
    assert np.array_equal(ranking_ref([5, 3, 9, 3]), [0, 3, 1])  # 9 dropped; the tie: higher label first


@pytest.mark.parametrize("hw", SIZES[:6])
def test_ccl_ref_matches_scipy(hw):
    ndi = pytest.importorskip("scipy.ndimage")
    h, w = hw
    for name, im in patterns(h, w).items():
        lab, areas = ccl_ref(im)
        exp, k = ndi.label(im != 0, structure=np.ones((3, 3)))
        assert np.array_equal(lab, exp), name
        assert len(areas) == k + 1 and np.array_equal(areas, np.bincount(exp.ravel(), minlength=k + 1)), name
        if name in ("serpentine", "spiral", "full") or (name == "checker" and min(h, w) > 1):
            assert k == 1, name
        if name == "lattice":
            assert k == N.load().o3dx_ccl2d_max_labels(w, h) == ((w + 1) // 2) * ((h + 1) // 2)


def test_patterns_are_what_they_claim():
    pat = patterns(129, 257)
    lab, areas = ccl_ref(pat["combs"])
    assert len(areas) == 3  # two combs
    first = np.argwhere(lab == 1)[0]
    ys, xs = np.nonzero(lab == 1)
    assert (first[0], first[1]) != (ys.min(), xs.min())  # first pixel not at the bounding box's corner
    assert ccl_ref(pat["anti_diag"])[1].size > 3 and ccl_ref(pat["main_diag"])[1].size > 3
    assert abs((pat["fill41"] != 0).mean() - 0.41) < 0.02


def test_entry_points_validate_before_touching_the_device():
    """EINVAL / ENOMEM / ENOTSUP and their messages, before any device call
    (so this runs without a GPU)."""
    L = N.load()
    v = ctypes.c_void_p(8)  # never dereferenced: the checks come first
    err = lambda: L.o3dx_last_error()  # noqa: E731
    wh = np.zeros(2, np.int64)
    whp = wh.ctypes.data_as(ctypes.c_void_p)
    b = np.array([0.0, 0.0, 1.0, 2.0])
    bp = b.ctypes.data_as(ctypes.c_void_p)
    # size
    assert L.o3dx_raster2d_size(0.1, bp, whp) == 0 and list(wh) == [10, 20]
    assert L.o3dx_raster2d_size(0.0, bp, whp) == -22 and b"resolution" in err()
    assert L.o3dx_raster2d_size(float("nan"), bp, whp) == -22 and b"resolution" in err()
    assert L.o3dx_raster2d_size(0.1, None, whp) == -22 and b"bounds" in err()
    assert L.o3dx_raster2d_size(0.1, bp, None) == -22 and b"wh_host" in err()
    bad = np.array([0.0, 0.0, np.inf, 2.0])
    assert L.o3dx_raster2d_size(0.1, bad.ctypes.data_as(ctypes.c_void_p), whp) == -22 and b"finite" in err()
    bad = np.array([0.0, 3.0, 1.0, 2.0])
    assert L.o3dx_raster2d_size(0.1, bad.ctypes.data_as(ctypes.c_void_p), whp) == -22 and b"max below min" in err()
    big = np.array([0.0, 0.0, 5000.0, 5000.0])
    bigp = big.ctypes.data_as(ctypes.c_void_p)
    assert L.o3dx_raster2d_size(0.1, bigp, whp) == -95 and b"2^31" in err()
    one = np.array([0.0, 0.0, 0.0, 2.0])  # one pixel column: w = 0 is the caller's to refuse
    assert L.o3dx_raster2d_size(0.1, one.ctypes.data_as(ctypes.c_void_p), whp) == 0 and list(wh) == [0, 20]
    # raster
    for fn, who in ((L.o3dx_raster2d, b"o3dx_raster2d"), (L.o3dx_raster2d_f64, b"o3dx_raster2d_f64")):
        assert fn(v, 0, 0.1, bp, v, v, None, 200, None) == -22 and who in err() and b"n = 0" in err()
        assert fn(v, 1 << 31, 0.1, bp, v, v, None, 200, None) == -22 and b"outside" in err()
        assert fn(None, 10, 0.1, bp, v, v, None, 200, None) == -22 and b"null" in err()
        assert fn(v, 10, 0.1, bp, None, v, None, 200, None) == -22 and b"null" in err()
        assert fn(v, 10, -1.0, bp, v, v, None, 200, None) == -22 and b"resolution" in err()
        assert fn(v, 10, 0.1, one.ctypes.data_as(ctypes.c_void_p), v, v, None, 200, None) == -22 and \
            b"empty image" in err()
        assert fn(v, 10, 0.1, bigp, v, v, None, 200, None) == -95 and b"2^31" in err()
        assert fn(v, 10, 0.1, bp, v, v, None, 199, None) == -12 and b"image buffer too small" in err()
    # labelling
    assert L.o3dx_ccl2d_max_labels(5, 3) == 6 and L.o3dx_ccl2d_max_labels(0, 3) == 0
    assert L.o3dx_ccl2d_workspace_bytes(100, 50) > 4 * 4 * 5000
    assert L.o3dx_ccl2d_workspace_bytes(0, 50) == 0 and L.o3dx_ccl2d_workspace_bytes(1 << 16, 1 << 15) == 0
    k = np.zeros(1, np.int64)
    kp = k.ctypes.data_as(ctypes.c_void_p)
    assert L.o3dx_ccl2d(v, 0, 5, v, v, kp, v, 1 << 30, None) == -22 and b"empty" in err()
    assert L.o3dx_ccl2d(v, 1 << 16, 1 << 15, v, v, kp, v, 1 << 30, None) == -95 and b"2^31" in err()
    assert L.o3dx_ccl2d(None, 10, 5, v, v, kp, v, 1 << 30, None) == -22 and b"null" in err()
    assert L.o3dx_ccl2d(v, 10, 5, v, v, None, v, 1 << 30, None) == -22 and b"null" in err()
    assert L.o3dx_ccl2d(v, 10, 5, v, v, kp, v, 16, None) == -12 and b"workspace" in err()
    assert L.o3dx_ccl2d(v, 10, 5, v, v, kp, None, 1 << 30, None) == -12 and b"workspace" in err()
    # grouping
    assert L.o3dx_label_group_workspace_bytes(1000, 7) > 8 * 1000
    assert L.o3dx_label_group_workspace_bytes(0, 7) == 0 and L.o3dx_label_group_workspace_bytes(10, -1) == 0
    assert L.o3dx_label_group(v, 0, v, 10, 5, 3, v, v, v, v, 1 << 30, None) == -22 and b"n = 0" in err()
    assert L.o3dx_label_group(v, 10, v, 0, 5, 3, v, v, v, v, 1 << 30, None) == -22 and b"image" in err()
    assert L.o3dx_label_group(v, 10, v, 10, 5, -1, v, v, v, v, 1 << 30, None) == -22 and b"n_labels" in err()
    assert L.o3dx_label_group(v, 10, None, 10, 5, 3, v, v, v, v, 1 << 30, None) == -22 and b"null" in err()
    assert L.o3dx_label_group(v, 10, v, 10, 5, 3, v, v, None, v, 1 << 30, None) == -22 and b"null" in err()
    assert L.o3dx_label_group(v, 10, v, 10, 5, 3, v, v, v, v, 16, None) == -12 and b"workspace" in err()


def test_python_argument_errors():
    """The checks that come before any device work."""
    pc = o3p.PointCloud(np.random.default_rng(0).random((50, 3)))
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            pc.to_2D_Img(bad)
    with pytest.raises(ValueError):
        o3p.PointCloud().to_2D_Img(0.1)
    nan = np.random.default_rng(0).random((50, 3))
    nan[7, 1] = np.nan
    with pytest.raises(ValueError):
        o3p.PointCloud(nan).to_2D_Img(0.1)
    nan[7, 1] = np.inf
    with pytest.raises(ValueError):
        o3p.PointCloud(nan).to_2D_Img(0.1)
    with pytest.raises(ValueError):
        o3p.ops.raster2d(torch.zeros((0, 3)), 0.1)
    with pytest.raises(ValueError):
        o3p.ops.raster2d(torch.zeros((5, 3)), -1.0)
    img = np.zeros((4, 6), np.uint8)
    ok = np.zeros((50, 2), np.int64)
    with pytest.raises(IndexError):
        pc.simple_seg_connected_components_by_img(img, 0, None, 0, None, 0.1, ok[:49])
    for x, y in ((6, 0), (0, 4), (-1, 0), (0, -1)):
        idx = ok.copy()
        idx[3] = (x, y)
        with pytest.raises(IndexError):
            pc.simple_seg_connected_components_by_img(img, 0, None, 0, None, 0.1, idx)
    with pytest.raises(ValueError):
        pc.simple_seg_connected_components_by_img(np.zeros((4, 6, 3), np.uint8), 0, None, 0, None, 0.1, ok)
    assert np.array_equal(o3p.PointCloud._ccl_ranking(np.array([5, 3, 9, 3])), [0, 3, 1])


@pytest.mark.skipif(GPU, reason="checks the no-GPU behaviour")
def test_compute_fails_loudly_without_gpu():
    pc = o3p.PointCloud(np.random.default_rng(0).random((50, 3)))
    with pytest.raises(RuntimeError):
        pc.to_2D_Img(0.1)
    with pytest.raises(RuntimeError):
        pc.simple_seg_connected_components([0, 0, 1, -0.5], 0.6)
    with pytest.raises(RuntimeError):
        o3p.ops.ccl2d(torch.zeros((4, 4), dtype=torch.uint8))


def test_processor_fields_and_json_roundtrip():
    p = o3p.Processors.SimpleSegConnectedComponents(thickness=0.07, top_n=5)
    assert p.title == "simple_seg_connected_components" and p.plane == [0, 0, 1.0, 0.0]
    assert (p.thickness, p.resolution, p.minpoints, p.top_n) == (0.07, 0.1, 20, 5)
    d = o3p.Processors.SimpleSegConnectedComponents()
    assert (d.thickness, d.resolution, d.minpoints, d.top_n) == (0.05, 0.1, 20, 100)
    assert p.uuid.split(":")[0] == "SimpleSegConnectedComponents"
    back = o3p.PointCloudMatProcessors.loads(o3p.PointCloudMatProcessors.dumps([p, o3p.Processors.DoingNothing()]))
    assert type(back[0]) is o3p.Processors.SimpleSegConnectedComponents
    assert back[0].uuid == p.uuid and back[0].thickness == 0.07 and back[0].top_n == 5
    from open3dpypro.PointCloudMat import ShapeType
    mats = p.build_out_mats([], [np.zeros((4, 3)), np.zeros((0, 3))])
    assert [m.info.shape_type for m in mats] == [ShapeType.XYZ, ShapeType.XYZ]
