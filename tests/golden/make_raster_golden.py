"""Writes tests/golden/raster_ref.npz: the rasterisation and selection cases
of tests/test_raster_ccl.py / tests/test_gpu_raster_ccl.py with the reference's
own answers.

    python tests/golden/make_raster_golden.py REFERENCE_DIR

REFERENCE_DIR holds the reference package (open3dpypro/PointCloud.py); it is
imported with open3d and cv2 mocked, as make_golden.py does.  Needs scipy; the
tests read only the file.

Rasterisation cases (r_<name>_*): the reference's unbound PointCloud.to_2D_Img
on a stub offering get_points / has_colors / get_colors.  Stored: the points
(float32 where the values are float32-exact), the resolution, the colours if
any, and the reference's img, ix, iy (idx2img's columns) and T.

Selection cases (s_<name>_*): the reference's simple_seg_connected_components
on a stub cloud whose _select_by_idx remembers original indices, with
cv2.connectedComponentsWithStats replaced by a stand-in on scipy.ndimage.label
(3x3 structure; the stats' last column is the pixel count, row 0 the
background).  The inputs are rectangular patches of pairwise distinct pixel
areas (asserted here, the background included: the reference's argsort is
unstable on ties), at least 2 empty pixels apart, plus off-plane clutter.
Stored: points, plane, thickness, resolution, minpoints, top_n and the returned
clouds' original indices (concatenated, with offsets).
"""
import os
import sys
import unittest.mock as mock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "raster_ref.npz")


def load_reference(ref_dir):
    sys.modules["open3d"] = mock.MagicMock()
    sys.modules["cv2"] = mock.MagicMock()
    sys.path.insert(0, ref_dir)
    from open3dpypro.PointCloud import PointCloud  # the reference package
    return PointCloud


def cc_standin(img):
    from scipy import ndimage as ndi
    labels, k = ndi.label(np.asarray(img) != 0, structure=np.ones((3, 3)))
    stats = np.zeros((k + 1, 5), np.int32)
    stats[:, -1] = np.bincount(labels.ravel(), minlength=k + 1)
    return k + 1, labels.astype(np.int32), stats, np.zeros((k + 1, 2))


def make_stub(Ref):
    class Stub:
        def __init__(self, pts, colors=None, orig=None):
            self.pts = np.asarray(pts, np.float64)
            self.colors = colors
            self.orig = np.arange(len(self.pts)) if orig is None else orig

        def get_points(self):
            return self.pts.copy()

        def has_colors(self):
            return self.colors is not None

        def get_colors(self):
            return np.asarray(self.colors, np.float64)

        def size(self):
            return len(self.pts)

        def _select_by_idx(self, idx, invert=False):
            mask = np.zeros(len(self.pts), bool)
            mask[np.asarray(idx, dtype=np.int64)] = True
            return Stub(self.pts[mask], None, self.orig[mask])

        _bool2index = Ref._bool2index
        get_index_by_plane = Ref.get_index_by_plane
        to_2D_Img = Ref.to_2D_Img
        simple_seg_connected_components = Ref.simple_seg_connected_components

    return Stub


def raster_cases():
    rng = np.random.default_rng(20250310)
    f32 = (rng.random((1000, 3)) * [7.0, 5.0, 1.0] + [-2.0, 3.0, 0.0]).astype(np.float32)
    yield "f32_r10", f32, 0.1, None
    yield "f32_r05", f32, 0.05, None
    wide = rng.random((1500, 3)) * [6.0, 4.0, 1.0] + [4.5e5, 4.5e5, 30.0]
    assert not np.array_equal(wide.astype(np.float32).astype(np.float64), wide)
    yield "f64_offset_r07", wide, 0.07, None
    # multiples of 1/8 from 0: x * 10 and x * 20 are exact, and k + 0.5 for even and odd k
    half = (rng.integers(0, 49, (800, 3)) / 8.0).astype(np.float32)
    half[0] = 0.0
    yield "half_r10", half, 0.1, None
    yield "half_r05", half, 0.05, None
    col = (rng.integers(0, 256, (1200, 3)) / 255.0).astype(np.float32)
    dense = (rng.random((1200, 3)) * [1.5, 1.2, 1.0]).astype(np.float32)
    yield "collide_r10", dense, 0.1, col
    yield "collide_r07", dense, 0.07, col


def patches(rng, rects, res, per_pixel, plane, n_clutter):
    """Points on the plane filling every pixel of the rectangles (x0, y0, nx, ny
    in pixels; per_pixel[i] points in each pixel of rectangle i), plus clutter
    well off the plane, shuffled."""
    a, b, c, d = plane
    parts = []
    for (x0, y0, nx, ny), pp in zip(rects, per_pixel):
        gx, gy = np.meshgrid(np.arange(x0, x0 + nx), np.arange(y0, y0 + ny))
        g = np.stack([gx.ravel(), gy.ravel()], 1).repeat(pp, axis=0).astype(np.float64)
        xy = (g + rng.uniform(-0.2, 0.2, g.shape)) * res
        z = -(a * xy[:, 0] + b * xy[:, 1] + d) / c + rng.uniform(-0.01, 0.01, len(xy))
        parts.append(np.c_[xy, z])
    ext = np.concatenate(parts)[:, :2].max(0)
    cl = rng.random((n_clutter, 3)) * [ext[0], ext[1], 1.0]
    cl[:, 2] = -(a * cl[:, 0] + b * cl[:, 1] + d) / c + rng.choice([-1, 1], n_clutter) * rng.uniform(0.3, 1.0, n_clutter)
    p = np.concatenate(parts + [cl])
    return p[rng.permutation(len(p))].astype(np.float32)


def select_cases():
    rng = np.random.default_rng(20250311)
    flat, tilt = np.array([0, 0, 1.0, -0.5]), np.array([-0.1, 0.05, 1.0, -0.5])
    # rectangles (x0, y0, nx, ny) in pixels, >= 2 empty pixels apart; the first starts at the origin pixel
    rects = [(0, 0, 9, 7), (12, 0, 5, 11), (20, 2, 4, 4), (0, 10, 8, 3), (11, 14, 13, 5), (27, 9, 3, 12)]
    yield "plain", patches(rng, rects[:5], 0.1, [2, 1, 3, 2, 1], tilt, 300), tilt, 0.05, 0.1, 20, 100
    big = [(0, 0, 22, 20), (25, 0, 3, 9), (25, 12, 4, 12), (0, 23, 10, 3)]
    yield "blob_over_background", patches(rng, big, 0.05, [1, 2, 1, 2], flat, 200), flat, 0.05, 0.05, 0, 100
    yield "minpoints", patches(rng, rects[:5], 0.07, [3, 3, 1, 3, 3], flat, 300), flat, 0.04, 0.07, 50, 100
    yield "top_n", patches(rng, rects, 0.1, [1, 2, 2, 1, 1, 2], tilt, 300), tilt, 0.05, 0.1, 5, 3


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    Ref = load_reference(sys.argv[1])
    Stub = make_stub(Ref)
    sys.modules["cv2"].connectedComponentsWithStats = cc_standin
    out = {}
    for name, pts, res, col in raster_cases():
        img, minx, T, miny, invT, r, idx2img = Stub(pts, col).to_2D_Img(res, color=col is not None)
        idx = np.asarray(idx2img)
        assert img.dtype == np.uint8 and img.ndim == (3 if col is not None else 2)
        out.update({f"r_{name}_pts": pts, f"r_{name}_res": res, f"r_{name}_img": img,
                    f"r_{name}_ix": idx[:, 0].astype(np.int32), f"r_{name}_iy": idx[:, 1].astype(np.int32),
                    f"r_{name}_T": T})
        if col is not None:
            out[f"r_{name}_col"] = col
        hits = len(np.unique(idx[:, 1] * img.shape[1] + idx[:, 0]))
        print(f"raster {name}: n={len(pts)} img={img.shape} hit pixels={hits}")
    for name, pts, plane, thick, res, minpoints, top_n in select_cases():
        cloud = Stub(pts)
        slab = cloud._select_by_idx(cloud.get_index_by_plane(plane, thick))
        img = slab.to_2D_Img(resolution=res)[0]
        _, _, stats, _ = cc_standin(img)
        areas = stats[:, -1]
        assert len(set(areas.tolist())) == len(areas), (name, areas)  # no ties, the background included
        res_clouds = cloud.simple_seg_connected_components(plane, thick, res, minpoints, top_n)
        idxs = [c.orig.astype(np.int32) for c in res_clouds]
        offs = np.concatenate([[0], np.cumsum([len(i) for i in idxs])]).astype(np.int64)
        out.update({f"s_{name}_pts": pts, f"s_{name}_plane": plane, f"s_{name}_thickness": thick,
                    f"s_{name}_res": res, f"s_{name}_minpoints": minpoints, f"s_{name}_top_n": top_n,
                    f"s_{name}_indices": np.concatenate(idxs) if idxs else np.zeros(0, np.int32),
                    f"s_{name}_offsets": offs})
        print(f"select {name}: n={len(pts)} slab={slab.size()} img={img.shape} areas={areas.tolist()} "
              f"clouds={[len(i) for i in idxs]}")
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 300 * 1024


if __name__ == "__main__":
    main()
