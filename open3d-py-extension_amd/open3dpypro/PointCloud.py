"""PointCloud — drop-in for open3dpypro.PointCloud (reference
/root/reference/open3dpypro/PointCloud.py), without Open3D.

Storage: points / normals / colors live on the GPU as float32 (N,3) torch
tensors (the kernels' input layout); a float64 host copy of the points is kept
when the caller supplied host data, so get_points() round-trips the caller's
values exactly, as Open3D's float64 storage does.  A float64 cloud that
float32 cannot hold (a LAS / E57 scan at a georeferenced offset; the check
runs once per set_points) also keeps a float64 device copy, and the hot-path
methods run the float64 kernels on it (ops / include/o3dx.h "float64
boundary"): voxel keys, kNN distances, normals' moments, RANSAC distances and
ICP are then computed from the float64 values, as Open3D computes them.
intensity / labels / row / column indices are plain numpy attributes, as in
the reference.

The hot-path methods call libo3dx.so (ops.py); there is no CPU fallback —
without an MI355X they raise RuntimeError.  Host-only helpers (selections by
numpy predicate, splitting, I/O) run anywhere.  DBSCAN (the reference's
sklearn call) runs on the GPU and returns sklearn's labels (ops.dbscan).
to_2D_Img and the floor-map segmentation (simple_seg_connected_components,
simple_seg_connected_components_by_img; the reference's cv2 labelling) run on
the GPU too: ops.raster2d / ccl2d / label_group.  estimate_normals(method=
"poisson") orients the stored normals on the GPU (Open3D's
orient_normals_consistent_tangent_plane: ops.orient_normals_tangent_plane).
LAS files (read_las, read_las_gen, save_las, append_save_las, pcd2las:
PointCloudAdvanceIO, las_io.py) are decoded and encoded on the GPU
(ops.las_unpack / las_pack) and by numpy without one.
E57 files (read_e57, read_e57_gen, read_e57_scan_gen, read_e57_gen_scan_gen,
save_e57, save_pcds_e57, e572las: e57_io.py, without pye57) have their page
checksums verified and their records decoded and encoded on the GPU
(ops.e57_crc_pages / e57_unpack / e57_pack / e57_seal), by numpy without one.
Out of scope (SURVEY.md §2
row 5) and not mirrored: the colour-cosine selections, the reference's
other cv2 methods (detect_3d_circles, read_single_RGB), compressed LAZ, E57
spherical coordinates and images2D, get_lasdata (it returns laspy objects), the
E57 scan index of save_las(pt_src_id=True) and the image I/O (save_png /
save_jpg / save_tiff).
"""
from __future__ import annotations

import os
import uuid
from typing import Callable, List, Tuple

import numpy as np
import torch

from . import e57_io, las_io, ops, pcd_io
from . import _native as N
from .params import (Feature, KDTreeSearchParamHybrid, KDTreeSearchParamKNN, RANSACConvergenceCriteria,
                     TransformationEstimationPointToPoint, resolve, resolve_checkers, resolve_estimation)

_SEED = [None]


def _sor_keep_sequential(avg: np.ndarray, nv: int, std_ratio: float) -> np.ndarray:
    """RemoveStatisticalOutliers' cloud statistics in Open3D's order:
    std::accumulate of the positive means, std::inner_product of their
    squared deviations (both sequential over the index), then the decision."""
    pos = avg > 0
    S = np.add.accumulate(np.where(pos, avg, 0.0))[-1]
    m = S / nv
    t = np.where(pos, (avg - m) * (avg - m), 0.0)
    sq = np.add.accumulate(t)[-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        std = np.sqrt(sq / np.float64(nv - 1))
    thr = m + std_ratio * std
    return np.nonzero(pos & (avg < thr))[0].astype(np.int64)


def set_random_seed(seed: int):
    """Counterpart of o3d.utility.random.seed: seeds segment_plane's sampler."""
    _SEED[0] = int(seed)


def _next_seed() -> int:
    if _SEED[0] is None:
        return int(np.random.SeedSequence().entropy) & 0xFFFFFFFF
    s = _SEED[0]
    _SEED[0] = (s * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
    return s & 0xFFFFFFFF


def _device() -> torch.device:
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")


def _as_np(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().numpy()
    return np.asarray(a)


def _f32_exact(a) -> bool:
    """Every value of the float64 array / tensor is a float32 value (NaN
    included): the float32 kernels then see exactly Open3D's float64 inputs."""
    if isinstance(a, torch.Tensor):
        t = a.detach()
        return bool(((t.float().double() == t) | torch.isnan(t)).all().item())
    with np.errstate(over="ignore", invalid="ignore"):
        return bool(np.array_equal(a.astype(np.float32).astype(np.float64), a, equal_nan=True))


def _check3(a, what):
    if a.ndim != 2 or a.shape[1] != 3:
        raise AssertionError(f"{what} shape must be (n,3)")


class RegistrationResult:
    """Mirror of o3d.pipelines.registration.RegistrationResult."""

    def __init__(self, transformation, fitness, inlier_rmse, correspondence_set):
        self.transformation = transformation
        self.fitness = fitness
        self.inlier_rmse = inlier_rmse
        self.correspondence_set = correspondence_set

    def __repr__(self):
        return (f"RegistrationResult with fitness={self.fitness:e}, inlier_rmse={self.inlier_rmse:e}, "
                f"and correspondence_set size of {len(self.correspondence_set)}")


class KDTreeGrid:
    """Stand-in for o3d.geometry.KDTreeFlann (reference PointCloud.py:148-163):
    the same search_* methods and return shapes (k, IntVector-like int64
    indices, DoubleVector-like float64 d^2).  Each call is one device query of
    any size (o3dx_search_one: a float64 d^2 pass over the cloud, the
    candidates compacted and radix-sorted by (d^2, index)) — the reference's
    get_points_by_knn asks for up to 10^6 neighbours."""

    def __init__(self, cloud: "PointCloudBase"):
        self._x = cloud._hot_points()

    def _one(self, query, mode, knn, radius):
        k, idx, d2 = ops.search_one(self._x, np.asarray(query, np.float64).reshape(3), mode=mode, knn=knn,
                                    radius=radius)
        return k, idx.cpu().numpy().astype(np.int64), d2.cpu().numpy()

    def search_knn_vector_3d(self, query, knn: int):
        return self._one(query, N.SEARCH_KNN, knn, 0.0)

    def search_hybrid_vector_3d(self, query, radius: float, max_nn: int):
        return self._one(query, N.SEARCH_HYBRID, max_nn, radius)

    def search_radius_vector_3d(self, query, radius: float):
        return self._one(query, N.SEARCH_RADIUS, 0, radius)


def _warn_offset_icp(src: "PointCloudBase", tgt: "PointCloudBase"):
    """Point-to-plane ICP forms J = p x n on the raw coordinates, so its 6x6
    normal matrix has entries ~|p|^2 against ~1: far from the origin relative
    to its extent (georeferenced LAS / E57 scans, ~5e5 m) the system is
    rounding noise in float64 — for Open3D as well (tests/test_oracle.py
    test_icp_offset_conditioning).  Warn; the remedy is to register in a
    re-centred frame (subtract a common origin from both clouds)."""
    import warnings

    mn, mx = src.get_aabb() if hasattr(src, "get_aabb") else (None, None)
    tmn, tmx = tgt.get_aabb() if hasattr(tgt, "get_aabb") else (None, None)
    if mn is None or tmn is None:
        return
    far = max(np.abs(np.asarray(mn)).max(), np.abs(np.asarray(mx)).max(), np.abs(np.asarray(tmn)).max(),
              np.abs(np.asarray(tmx)).max())
    ext = max(float(np.max(np.asarray(mx) - np.asarray(mn))), float(np.max(np.asarray(tmx) - np.asarray(tmn))), 1e-12)
    if far / ext > 1e3:
        warnings.warn(f"registration_icp: the clouds lie {far:.3g} from the origin at an extent of {ext:.3g}; "
                      "point-to-plane ICP on raw coordinates that far out is ill-conditioned in float64 (Open3D's "
                      "too): register in a re-centred frame", RuntimeWarning, stacklevel=3)


class PointCloudBase:
    COLOR_CHART = np.asarray([[230, 0, 18], [243, 152, 0], [252, 200, 0], [143, 195, 31], [0, 153, 68],
                              [0, 160, 233], [29, 32, 136], [146, 7, 131], [228, 0, 127]])

    def __init__(self, xyz=None, rgb=None, normals=None, intensity=None, labels=None, row_index=None,
                 column_index=None, e57=None):
        self.e57 = e57          # the E57File of read_e57 (e57_io.E57File)
        self.intensity = []
        self.labels = []
        self.row_index = []
        self.column_index = []
        self._pts = None        # (N,3) float32 tensor on the device
        self._pts_host = None   # (N,3) float64 exact host copy (when supplied from host)
        self._pts64 = None      # device float64 copy of _pts_host (plane selections), made on demand
        # _wide: SOME float64 value is not float32-representable, so every hot
        # op runs its float64 kernels (o3dx_*_f64) to keep Open3D's float64
        # arithmetic on the exact values.  This is not limited to georeferenced
        # scans: np.random float64 arrays and a cloud after transform() with a
        # general rotation (transform() re-calls set_points) qualify too.  The
        # float64 path is slower (normals ~2-4x) and keeps no
        # voxel table for the normals.  Pass float32 values (or
        # points.astype(np.float32)) to opt into the float32 kernels: Open3D's
        # result on those values is the same either way.
        self._wide = False
        self._normals = None    # (N,3) float32 tensor
        self._colors = None     # (N,3) float32 tensor in [0,1]
        self.pcd_tree = None
        self.scan_No = -1
        self.uuid = uuid.uuid4()

        if isinstance(xyz, PointCloudBase):
            self._copy_from(xyz)
            return
        if xyz is not None and hasattr(xyz, "points") and not isinstance(xyz, (np.ndarray, torch.Tensor)):
            # an open3d.geometry.PointCloud (or anything shaped like one)
            pts = np.asarray(xyz.points)
            normals = np.asarray(xyz.normals) if len(getattr(xyz, "normals", [])) else normals
            rgb = np.asarray(xyz.colors) if len(getattr(xyz, "colors", [])) else rgb
            xyz = pts

        def ok(a):
            return a is not None and len(a) > 0 and np.prod(a.shape) > 0

        if ok(intensity):
            self.set_intensity(intensity)
        if ok(labels):  # accepted but silently dropped by the reference's __init__
            self.set_labels(labels)
        if ok(row_index):
            self.row_index = row_index
        if ok(column_index):
            self.column_index = column_index
        if ok(xyz):
            self.set_points(xyz)
        if ok(normals):
            self.set_normals(normals)
        if ok(rgb):
            self._set_rgb_rescaled(rgb)

    def _set_rgb_rescaled(self, rgb):
        """The constructor's colour rule: values outside [0, 1] are min-max rescaled."""
        rgb = _as_np(rgb)
        if rgb.max() > 1.0 or rgb.min() < 0.0:   # reference PointCloud.py:36-40
            rgb = rgb * 1.0
            rgb = (rgb - rgb.min()) / (rgb.max() - rgb.min())
        self.set_rgb(rgb)

    # ----------------------------------------------------------- storage
    def _copy_from(self, other: "PointCloudBase"):
        self._pts = other._pts
        self._pts_host = other._pts_host
        self._pts64 = other._pts64
        self._wide = other._wide
        self._normals = other._normals
        self._colors = other._colors
        self.intensity = other.intensity
        self.labels = other.labels
        self.row_index = other.row_index
        self.column_index = other.column_index

    def _dev_points(self) -> torch.Tensor:
        """float32 (N,3) device tensor — the kernels' input."""
        if self._pts is None:
            return torch.zeros((0, 3), dtype=torch.float32, device=_device())
        if self._pts.device.type != "cuda" and torch.cuda.is_available():
            self._pts = self._pts.to(_device())
        return self._pts

    def _plane_points(self) -> torch.Tensor:
        """The coordinates the plane selections evaluate: the caller's exact
        float64 values when the cloud came from float64 data (the reference
        computes distance2plane on get_points(), float64: PointCloud.py:
        400-404), else the float32 device points."""
        if self._pts_host is None and self._pts64 is None:
            return self._dev_points()
        if self._pts64 is None or self._pts64.device.type != "cuda":
            src = self._pts_host if self._pts_host is not None else self._pts64
            self._pts64 = torch.as_tensor(src, dtype=torch.float64, device=N.default_device())
        return self._pts64

    def _hot_points(self) -> torch.Tensor:
        """The hot-path kernels' input: the float64 device copy when float32
        cannot hold the cloud's values (the o3dx_*_f64 entry points, Open3D's
        float64 arithmetic), else the float32 device points (identical
        inputs: every float64 value is a float32 value)."""
        return self._plane_points() if self._wide else self._dev_points()

    @staticmethod
    def _to_dev(a, dtype=torch.float32) -> torch.Tensor:
        if isinstance(a, torch.Tensor):
            t = a.detach()
            if t.device.type == "cpu" and torch.cuda.is_available():
                t = t.to(_device())
            return t.to(dtype).contiguous()
        return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=_device())

    def clear(self):
        self.__init__()
        return self

    def size(self) -> int:
        return 0 if self._pts is None else int(self._pts.shape[0])

    def has_points(self) -> bool:
        return self.size() > 0

    def is_empty(self) -> bool:
        return not self.has_points()

    def has_colors(self) -> bool:
        return self._colors is not None and len(self._colors) > 0

    def get_center(self) -> np.ndarray:
        return self.get_points().mean(0) if self.has_points() else np.zeros(3)

    def transform(self, T: np.ndarray):
        """p <- (T @ [p;1])[:3] / w ; normals <- R n (Open3D Geometry3D::Transform)."""
        T = np.asarray(T, np.float64).reshape(4, 4)
        if self.has_points():
            if self._pts_host is not None:
                h = self._pts_host @ T[:3, :3].T + T[:3, 3]  # set_points drops _pts64
                w = self._pts_host @ T[3, :3] + T[3, 3]
                self.set_points(h / w[:, None])
            elif self._pts64 is not None:
                Tt = torch.as_tensor(T, dtype=torch.float64, device=self._pts64.device)
                h = self._pts64 @ Tt[:3, :3].T + Tt[:3, 3]
                w = self._pts64 @ Tt[3, :3] + Tt[3, 3]
                self.set_points(h / w[:, None])
            else:
                Tt = torch.as_tensor(T, dtype=torch.float64, device=self._pts.device)
                p = self._pts.double()
                h = p @ Tt[:3, :3].T + Tt[:3, 3]
                w = p @ Tt[3, :3] + Tt[3, 3]
                self._pts = (h / w[:, None]).float().contiguous()
        if self._normals is not None:
            R = torch.as_tensor(T[:3, :3], dtype=torch.float64, device=self._normals.device)
            self._normals = (self._normals.double() @ R.T).float().contiguous()
        self.pcd_tree = None
        return self

    def translate(self, t: np.ndarray, relative: bool = True):
        t = np.asarray(t, np.float64).reshape(3)
        if not relative:
            t = t - self.get_center()
        T = np.eye(4)
        T[:3, 3] = t
        return self.transform(T)

    def rotate(self, R: np.ndarray, center=None):
        R = np.asarray(R, np.float64).reshape(3, 3)
        c = self.get_center() if center is None else np.asarray(center, np.float64)
        T = np.eye(4)
        T[:3, :3] = R
        T[:3, 3] = c - R @ c
        return self.transform(T)

    # ------------------------------------------------------------ hot path
    def estimate_normals(self, method="default", param=KDTreeSearchParamKNN(30)):
        """Open3D EstimateNormals(param, fast_normal_computation=True) on the GPU
        (reference PointCloud.py:68-73).  Existing normals orient the result."""
        if method == "poisson":  # reference PointCloud.py:69-70
            return self.orient_normals_consistent_tangent_plane(k=30)
        mode, knn, radius = resolve(param)
        x = self._hot_points()
        prior = self._normals if self.has_normals() else None
        self._normals = ops.estimate_normals(x, mode=mode, knn=knn, radius=radius, prior=prior,
                                             voxel_grid=None if self._wide else self._kept_voxel_grid(x))
        return self

    def orient_normals_consistent_tangent_plane(self, k: int = 30):
        """Open3D OrientNormalsConsistentTangentPlane(k) on the GPU
        (ops.orient_normals_tangent_plane; include/o3dx.h states the rule):
        the stored normals keep their magnitudes and get consistent signs
        along the minimum spanning tree of the Riemannian graph (k nearest
        neighbours united with the Euclidean MST), rooted at the highest
        point.  Returns self.  An empty cloud is left as it is; RuntimeError,
        as Open3D, for a cloud without normals; ValueError for k < 1 or
        non-finite coordinates, all before any GPU work.  Fewer than 4 or coplanar points work (Open3D's
        Qhull step fails there); Open3D 0.18+'s lambda / cos_alpha_tol are
        not offered.  float64 clouds that float32 cannot hold raise
        NotImplementedError."""
        if not self.has_points():
            return self
        if not self.has_normals():
            raise RuntimeError("No normals in the PointCloud. Call EstimateNormals() first.")
        if int(k) != k or int(k) < 1:
            raise ValueError(f"k must be an int >= 1, got {k}")
        if self._wide:
            raise NotImplementedError("orient_normals_consistent_tangent_plane: float64 clouds that float32 cannot "
                                      "hold are outside this implementation (pass float32 values)")
        if not self._finite_points():
            raise ValueError("orient_normals_consistent_tangent_plane: the coordinates must be finite")
        self._normals = ops.orient_normals_tangent_plane(self._dev_points(), self._normals, int(k))
        return self

    def _exact_points_like(self, t: torch.Tensor) -> torch.Tensor:
        """get_points()'s float64 values as a tensor on t's device."""
        if self._pts_host is not None:
            return torch.as_tensor(self._pts_host, dtype=torch.float64, device=t.device)
        if self._pts64 is not None:
            return self._pts64.to(t.device)
        return self._pts.to(t.device).double()

    def orient_normals_to_align_with_direction(self, orientation_reference=(0.0, 0.0, 1.0)):
        """Open3D OrientNormalsToAlignWithDirection: a zero normal becomes the
        reference, any other is negated iff n . ref < 0.  Returns self."""
        if not self.has_normals():
            raise RuntimeError("No normals in the PointCloud. Call EstimateNormals() first.")
        n = self._normals
        ref = torch.as_tensor(np.asarray(orientation_reference, np.float64).reshape(3), device=n.device)
        nd = n.double()
        zero = (nd == 0).all(dim=1, keepdim=True)
        flip = ((nd * ref).sum(dim=1, keepdim=True) < 0)
        out = torch.where(flip, -n, n)
        self._normals = torch.where(zero, ref.float().expand_as(n), out).contiguous()
        return self

    def orient_normals_towards_camera_location(self, camera_location=(0.0, 0.0, 0.0)):
        """Open3D OrientNormalsTowardsCameraLocation, ref = camera - point: a
        zero normal becomes ref normalised ((0, 0, 1) when ref is zero too), any
        other is negated iff n . ref < 0.  Returns self."""
        if not self.has_normals():
            raise RuntimeError("No normals in the PointCloud. Call EstimateNormals() first.")
        n = self._normals
        cam = torch.as_tensor(np.asarray(camera_location, np.float64).reshape(3), device=n.device)
        ref = cam - self._exact_points_like(n)
        nd = n.double()
        zero = (nd == 0).all(dim=1, keepdim=True)
        flip = ((nd * ref).sum(dim=1, keepdim=True) < 0)
        out = torch.where(flip, -n, n)
        norm = ref.norm(dim=1, keepdim=True)
        up = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64, device=n.device).expand_as(ref)
        fill = torch.where(norm == 0, up, ref / torch.where(norm == 0, torch.ones_like(norm), norm))
        self._normals = torch.where(zero, fill.float(), out).contiguous()
        return self

    def _kept_voxel_grid(self, x):
        """The voxel table of the voxel_down_sample that made this cloud, while
        its points are unchanged (same tensor, no in-place writes)."""
        kept = getattr(self, "_voxel_grid", None)
        if kept is None:
            return None
        vg, pts, version = kept
        if x is not pts or pts._version != version or vg.m != x.shape[0]:
            self._voxel_grid = None
            return None
        return vg

    def segment_plane(self, thickness: float = 0.01, ransac_n: int = 3, num_iterations: int = 450,
                      probability: float = 0.99999999, seed=None, samples=None) -> Tuple[List, List[int]]:
        """Open3D SegmentPlane (reference PointCloud.py:75-77) -> ([a,b,c,d], inlier indices)."""
        plane, inl = self._segment_plane_dev(thickness, ransac_n, num_iterations, probability, seed, samples)
        return plane, inl.cpu().numpy().astype(np.int64).tolist()

    def _segment_plane_dev(self, thickness=0.01, ransac_n=3, num_iterations=450, probability=0.99999999, seed=None,
                           samples=None):
        """segment_plane with the inlier indices left on the device (int32)."""
        x = self._hot_points()
        n = x.shape[0]
        if samples is None and n >= ransac_n >= 3 and 0 < probability <= 1:
            samples = ops.ransac_samples(n, ransac_n, num_iterations, _next_seed() if seed is None else seed)
        plane, inl = ops.segment_plane(x, thickness, ransac_n, num_iterations, probability, samples=samples)
        return [float(v) for v in plane], inl

    def get_aabb(self):
        if not self.has_points():
            return np.zeros(3), np.zeros(3)
        if self._pts_host is not None and not torch.cuda.is_available():
            raise RuntimeError("get_aabb needs the ROCm GPU (no CPU path)")
        return ops.aabb(self._hot_points())

    # ---------------------------------------------------------------- has
    def has_rgb(self) -> bool:
        return self.has_points() and self._colors is not None and self.size() == len(self._colors)

    def has_normals(self) -> bool:
        return self.has_points() and self._normals is not None and self.size() == len(self._normals)

    def has_intensity(self) -> bool:
        return self.has_points() and self.size() == len(self.intensity)

    def has_labels(self) -> bool:
        return self.has_points() and self.size() == len(self.labels)

    def has_col_row(self) -> bool:
        return self.has_points() and self.size() == len(self.column_index) == len(self.row_index)

    # ---------------------------------------------------------- set / get
    def set_rgb(self, colors):
        c = colors if isinstance(colors, torch.Tensor) else np.asarray(colors)
        _check3(c, "colors")
        self._colors = self._to_dev(c)
        return self

    def set_points(self, points):
        if isinstance(points, torch.Tensor):
            _check3(points, "points")
            self._pts_host = None
            self._pts64 = None
            self._wide = points.dtype == torch.float64 and not _f32_exact(points)
            if self._wide:  # kept in float64 on the device (get_points returns it)
                self._pts64 = self._to_dev(points, torch.float64)
            self._pts = self._to_dev(points)
        else:
            p = np.asarray(points)
            _check3(p, "points")
            self._pts_host = np.ascontiguousarray(p, dtype=np.float64)
            self._pts64 = None
            self._wide = not _f32_exact(self._pts_host)
            self._pts = self._to_dev(self._pts_host.astype(np.float32))
        self.pcd_tree = None
        return self

    def set_normals(self, normals):
        nrm = normals if isinstance(normals, torch.Tensor) else np.asarray(normals)
        _check3(nrm, "normals")
        self._normals = self._to_dev(nrm)
        return self

    def set_intensity(self, intensity: np.ndarray):
        assert intensity.shape[1] == 1, "intensity shape must be (n,1)"
        self.intensity = intensity
        return self

    def set_labels(self, labels: np.ndarray):
        assert labels.shape[1] == 1, "labels shape must be (n,1)"
        self.labels = labels
        return self

    def get_points(self) -> np.ndarray:
        if self._pts_host is not None:
            return self._pts_host.copy()
        if self._pts64 is not None:
            return self._pts64.detach().cpu().numpy().copy()
        if self._pts is None:
            return np.zeros((0, 3))
        return self._pts.detach().cpu().numpy().astype(np.float64)

    def get_colors(self) -> np.ndarray:
        return np.zeros((0, 3)) if self._colors is None else self._colors.cpu().numpy().astype(np.float64)

    def get_normals(self) -> np.ndarray:
        return np.zeros((0, 3)) if self._normals is None else self._normals.cpu().numpy().astype(np.float64)

    def get_intensity(self):
        return self.intensity

    def get_labels(self):
        return self.labels

    def get_col_row(self):
        return (self.column_index, self.row_index)

    def set_uniform_label(self, label: int):
        self.labels = np.ones((self.size(), 1), dtype=int) * label
        return self

    def set_uniform_intensity(self, intensity: float):
        self.set_intensity(np.ones((self.size(), 1), dtype=int) * intensity)
        return self

    # ------------------------------------------------------------- KD-tree
    def calc_KDtree(self):
        self.pcd_tree = KDTreeGrid(self)
        return self.pcd_tree

    def get_KDtree(self):
        if self.pcd_tree is None:
            self.calc_KDtree()
        return self.pcd_tree

    def get_points_by_knn(self, point_idx: int, max_nn: int = 1000000):
        q = self.get_points()[point_idx]
        return self.get_KDtree().search_knn_vector_3d(q, max_nn)

    def get_points_radius(self, point_idx: int, search_radius: float = 30.0):
        q = self.get_points()[point_idx]
        return self.get_KDtree().search_radius_vector_3d(q, search_radius)

    # ------------------------------------------------------------------ IO
    def read_pcd(self, filename: str, format: str = "auto", remove_nan_points: bool = False,
                 remove_infinite_points: bool = False, print_progress: bool = False):
        ext = (os.path.splitext(filename)[1].lstrip(".") if format == "auto" else format).lower()
        nrm = col = None
        if ext == "pcd" and torch.cuda.is_available():
            # decoded on the GPU into the device arrays the cloud keeps
            pts, nrm, col = pcd_io.read_pcd_device(filename, _device(), remove_nan_points, remove_infinite_points)
        elif ext == "pcd":
            pts, nrm, col = pcd_io.read_pcd(filename, remove_nan_points, remove_infinite_points)
        elif ext == "npy":
            pts = np.load(filename, allow_pickle=False).reshape(-1, 3).astype(np.float64)
        elif ext in ("xyz", "xyzn", "xyzrgb", "pts", "txt"):
            a = np.loadtxt(filename, ndmin=2)
            pts = a[:, :3]
            if ext == "xyzn" and a.shape[1] >= 6:
                nrm = a[:, 3:6]
            if ext == "xyzrgb" and a.shape[1] >= 6:
                col = a[:, 3:6]
        else:
            raise RuntimeError(f"read_pcd: unsupported format {ext!r}")
        if ext != "pcd" and (remove_nan_points or remove_infinite_points):
            keep = np.ones(len(pts), bool)
            if remove_nan_points:
                keep &= ~np.isnan(pts).any(1)
            if remove_infinite_points:
                keep &= ~np.isinf(pts).any(1)
            pts = pts[keep]
            nrm = nrm[keep] if nrm is not None else None
            col = col[keep] if col is not None else None
        return self.__class__(pts, rgb=col, normals=nrm)

    def save_pcd(self, filename: str, write_ascii: bool = False, compressed: bool = False,
                 print_progress: bool = False):
        return pcd_io.write_pcd(filename, self.get_points(), self.get_normals() if self.has_normals() else None,
                                self.get_colors() if self.has_rgb() else None, write_ascii=write_ascii)

    def draw(self, geos=[], point_size: int = 1, centralize: bool = False):
        raise NotImplementedError("visualisation is outside the GPU hot path (reference PointCloud.py:172-178)")


class PointCloudSelections(PointCloudBase):

    def clone(self, invert: bool = False):
        return self._select_by_idx(np.arange(self.size()), invert=invert)

    def _select_by_idx(self, indices, invert: bool = False):
        """Boolean-mask gather of every per-point attribute; output keeps ascending
        original index order (reference PointCloud.py:185-204)."""
        res = self.__class__()
        n = self.size()
        if isinstance(indices, torch.Tensor):
            dev = self._pts.device if self._pts is not None else indices.device
            mask = torch.zeros(n, dtype=torch.bool, device=dev)
            if indices.numel():
                mask[indices.to(dev).long()] = True
        else:
            idx = np.asarray(indices, dtype=np.int64).reshape(-1)
            mask = torch.zeros(n, dtype=torch.bool, device=self._pts.device if self._pts is not None else "cpu")
            if idx.size:
                mask[torch.as_tensor(idx, device=mask.device)] = True
        if invert:
            mask = ~mask
        sel = torch.nonzero(mask).reshape(-1)
        if self.has_points():
            res._pts = self._pts.index_select(0, sel).contiguous()
            res._wide = self._wide
            if self._pts_host is not None:
                res._pts_host = self._pts_host[sel.cpu().numpy()]
            elif self._pts64 is not None:
                res._pts64 = self._pts64.index_select(0, sel.to(self._pts64.device)).contiguous()
        if self.has_rgb():
            res._colors = self._colors.index_select(0, sel.to(self._colors.device)).contiguous()
        if self.has_normals():
            res._normals = self._normals.index_select(0, sel.to(self._normals.device)).contiguous()
        hm = None
        if self.has_intensity() or self.has_labels():
            hm = mask.cpu().numpy()
        if self.has_intensity():
            res.intensity = self.intensity[hm].copy()
        if self.has_labels():
            res.labels = self.labels[hm].copy()
        return res

    def select_by_box(self, center, x_direction, y_direction, z_direction, invert: bool = False):
        dirs = [np.asarray(d, np.float64) / np.linalg.norm(d) for d in (x_direction, y_direction, z_direction)]
        half = [np.linalg.norm(d) ** 2 for d in dirs]
        v = self.get_points() - np.asarray(center)
        inside = np.logical_and.reduce([np.square(v @ d) < h for d, h in zip(dirs, half)])
        return self.select_by_bool(inside, invert=invert)

    def _bool2index(self, bools, invert: bool = False) -> np.ndarray:
        b = np.asarray(bools)
        if invert:
            b = np.logical_not(b)
        return np.where(b)[0]

    def select_by_bool(self, bools, invert: bool = False):
        return self._select_by_idx(self._bool2index(bools), invert=invert)

    def get_index_by_normals(self, comfunc: Callable = lambda ns: np.ones(len(ns), dtype=bool), invert=False):
        if not self.has_normals():
            self.estimate_normals()
        return self._bool2index(comfunc(self.get_normals()), invert=invert)

    def select_by_normals(self, comfunc: Callable = lambda ns: np.ones(len(ns), dtype=bool), invert=False):
        return self._select_by_idx(self.get_index_by_normals(comfunc=comfunc), invert=invert)

    @staticmethod
    def _cosine(model, similarity):
        m = np.asarray(model, np.float64)[:3]
        return lambda v: (v @ m) / (np.linalg.norm(v, axis=1) * np.linalg.norm(m)) >= similarity

    def get_index_by_normals_cosine(self, model, similarity: float = 0.99, invert: bool = False):
        return self.get_index_by_normals(comfunc=self._cosine(model, similarity), invert=invert)

    def select_by_normals_cosine(self, model, similarity: float = 0.99, invert: bool = False):
        return self._select_by_idx(self.get_index_by_normals_cosine(model, similarity), invert=invert)

    def get_index_by_colors(self, comfunc: Callable = lambda rgb: np.ones(len(rgb), dtype=bool), invert=False):
        return self._bool2index(comfunc(self.get_colors()), invert=invert)

    def get_index_by_XYZ(self, comfunc: Callable = lambda X, Y, Z: np.ones(len(X), dtype=bool), invert=False):
        p = self.get_points()
        return self._bool2index(comfunc(p[:, 0], p[:, 1], p[:, 2]), invert=invert)

    def select_by_XYZ(self, comfunc: Callable = lambda X, Y, Z: np.ones(len(X), dtype=bool), invert=False):
        return self._select_by_idx(self.get_index_by_XYZ(comfunc), invert=invert)

    def get_index_by_radius(self, r: float, invert: bool = False):
        return self.get_index_by_XYZ(lambda X, Y, Z: (X ** 2 + Y ** 2 + Z ** 2) ** 0.5 <= r, invert=invert)

    def select_by_radius(self, r: float, invert: bool = False):
        return self._select_by_idx(self.get_index_by_radius(r), invert=invert)

    def get_index_by_plane(self, model, thickness=0.03, invert: bool = False):
        """|s| < thickness (strict), or a (lo, hi) signed band, s the point's
        signed distance to the plane (reference PointCloud.py:278-290), decided
        on the GPU (o3dx_plane_select) in float64; ascending numpy indices."""
        return self._plane_index_dev(model, thickness, invert).cpu().numpy().astype(np.int64)

    def _plane_index_dev(self, model, thickness, invert: bool = False) -> torch.Tensor:
        if not self.has_points():
            return torch.zeros(0, dtype=torch.int32, device=_device())
        return ops.plane_select(self._plane_points(), np.asarray(model, np.float64).reshape(4), thickness, invert)

    def select_by_plane(self, model, thickness=0.03, invert: bool = False):
        # indices stay on the device (reference PointCloud.py:289-290)
        return self._select_by_idx(self._plane_index_dev(model, thickness), invert=invert)

    def get_index_by_aabb(self, aabb_min, aabb_max, invert: bool = False):
        p = self.get_points()
        inside = np.all((p >= np.asarray(aabb_min)) & (p <= np.asarray(aabb_max)), axis=1)
        return self._bool2index(inside, invert=invert)

    def select_by_aabb(self, aabb_min, aabb_max, invert: bool = False):
        return self._select_by_idx(self.get_index_by_aabb(aabb_min, aabb_max), invert=invert)

    def get_index_by_aabb_list(self, aabb_min_max_list, invert: bool = False):
        p = self.get_points()
        inside = np.zeros(len(p), bool)
        for lo, hi in aabb_min_max_list:
            inside |= np.all((p >= np.asarray(lo)) & (p <= np.asarray(hi)), axis=1)
        return self._bool2index(inside, invert=invert)

    def select_by_aabb_list(self, aabb_min_max_list, invert: bool = False):
        return self._select_by_idx(self.get_index_by_aabb_list(aabb_min_max_list), invert=invert)

    def select_by_topN(self, n: int):
        return self._select_by_idx(np.arange(self.size())[:n])


class PointCloudUtility(PointCloudSelections):

    def paint_uniform_color(self, color=(1.0, 0.0, 0.0)):
        self._colors = self._to_dev(np.tile(np.asarray(color, np.float32).reshape(1, 3), (self.size(), 1)))
        return self

    def split_by_labels(self):
        ul = np.unique(self.labels)
        return [self.select_by_bool((self.labels == j).reshape(-1)) for j in ul], ul

    def centralize(self):
        return self.translate(-self.get_center())

    def voxel_down_sample_and_trace(self, voxel_size: float):
        """Open3D VoxelDownSampleAndTrace(vs, AABB min, AABB max) + idxmat.max(1) +
        _select_by_idx (reference PointCloud.py:338-341) on the GPU.

        Returns (cloud of the representatives in ascending index order,
        idxmat (M,8) int32 cubic-id matrix, vec: list of M int arrays).  Row r
        of idxmat / vec is the voxel of representative r; Open3D emits rows in
        its hash-map order instead, which no implementation can reproduce."""
        x = self._hot_points()
        mn, mx = self.get_aabb()
        out = ops.voxel_down_sample(x, voxel_size, mn, mx, with_xyz=False, trace=True)
        rep = out["rep_idx"]
        idxmat = out["cubic_id"].cpu().numpy()
        vop = out["voxel_of_point"].long()
        order = torch.argsort(vop, stable=True)
        counts = torch.bincount(vop, minlength=rep.numel()).cpu().numpy()
        flat = order.to(torch.int32).cpu().numpy()
        vec = np.split(flat, np.cumsum(counts)[:-1]) if rep.numel() else []
        return self._select_by_idx(rep), idxmat, vec

    def voxel_down_sample(self, voxel_size: float):
        """Representatives only (no trace) — the fast path."""
        x = self._hot_points()
        mn, mx = self.get_aabb()
        out = ops.voxel_down_sample(x, voxel_size, mn, mx, with_xyz=False, keep_grid=True)
        res = self._select_by_idx(out["rep_idx"])
        if out["voxel_grid"] is not None and res._pts is not None:
            # estimate_normals on the result reads its search grid off the voxel table
            res._voxel_grid = (out["voxel_grid"], res._pts, res._pts._version)
        return res

    def random_down_sample(self, down_sample_ratio: float = 0.1):
        if down_sample_ratio <= 0 or down_sample_ratio > 1:
            return self.__class__()
        idx = np.arange(self.size())
        np.random.shuffle(idx)
        return self._select_by_idx(idx[: int(len(idx) * down_sample_ratio)])

    def uniform_down_sample(self, down_sample_ratio: float = 0.1):
        if down_sample_ratio <= 0 or down_sample_ratio > 1:
            return self.__class__()
        return self._select_by_idx(np.arange(self.size())[:: int(1 / down_sample_ratio)])

    # scale of the rounding band around the outlier threshold (tests raise it
    # to force the exact sequential re-decision on every call)
    _SOR_BAND_SCALE = 8.0

    def remove_statistical_outlier(self, nb_neighbors: int = 20, std_ratio: float = 2.0,
                                   print_progress: bool = False):
        """Open3D RemoveStatisticalOutliers (reference PointCloud.py:370-372),
        index-exact: per point the mean of sqrt(d2) over its nb_neighbors
        nearest (self included), summed sequentially in ascending-distance
        order on the GPU (float64, the kernel's exact d2); keep points with
        0 < mean < cloud_mean + std_ratio * std (Bessel-corrected).

        Open3D forms cloud_mean and std with sequential std::accumulate /
        std::inner_product over all points in index order.  The GPU reduces
        them in a different order; their difference is bounded (a rounding
        band around the threshold).  When no point's mean lies inside that
        band the GPU decision is Open3D's; otherwise the two statistics are
        re-formed in Open3D's sequential order on the host (np.add.accumulate)
        and every point is decided against that threshold."""
        if nb_neighbors < 1 or std_ratio <= 0:
            raise RuntimeError("Illegal input parameters, the number of neighbors and standard deviation "
                               "ratio must be positive.")
        if not self.has_points():
            return self.__class__(), []
        x = self._hot_points()
        idx, d2, cnt = ops.knn_search(x, x, mode=N.SEARCH_KNN, knn=nb_neighbors)
        n = x.shape[0]
        col = torch.arange(d2.shape[1], device=d2.device)
        d = torch.where(col[None, :] < cnt[:, None].long(), torch.sqrt(d2.clamp_min(0)), torch.zeros_like(d2))
        acc = torch.zeros(n, dtype=torch.float64, device=d2.device)
        for j in range(d.shape[1]):  # std::accumulate order: ascending distance
            acc = acc + d[:, j]
        valid = cnt > 0
        avg = torch.where(valid, acc / cnt.clamp_min(1).double(), torch.full_like(acc, -1.0))
        nv = int(valid.sum().item())
        if nv == 0:
            return self.__class__(), []
        pos = avg > 0
        S = float(torch.where(pos, avg, torch.zeros_like(avg)).sum().item())
        m = S / nv
        sq = float(torch.where(pos, (avg - m) * (avg - m), torch.zeros_like(avg)).sum().item())
        std = float(np.sqrt(sq / (nv - 1))) if nv > 1 else float("nan")
        thr = m + std_ratio * std
        # |GPU order - sequential order| bounds (first order, n-term sums)
        E = (n + 4) * np.ldexp(1.0, -53)
        dm = 2.0 * E * m
        dsq = 2.0 * E * sq + 2.0 * dm * np.sqrt(max(n, 1) * sq)
        dstd = (std * (dsq / (2.0 * sq) + E)) if sq > 0 and np.isfinite(std) else 2.0 * np.sqrt(dsq / max(nv - 1, 1))
        band = self._SOR_BAND_SCALE * (dm + std_ratio * dstd) + abs(thr) * np.ldexp(1.0, -50)
        near = int((pos & ((avg - thr).abs() <= band)).sum().item()) if np.isfinite(thr) else 0
        if near == 0:
            keep = torch.nonzero(pos & (avg < thr)).reshape(-1)
        else:
            a = avg.cpu().numpy()
            keep = torch.from_numpy(_sor_keep_sequential(a, nv, std_ratio)).to(x.device)
        kept = keep.cpu().numpy().tolist()
        return self._select_by_idx(keep), kept

    def _require_finite_points(self, what: str):
        """ValueError when a coordinate is NaN or infinite (checked where the
        points live; a host cloud needs no GPU for it)."""
        src = self._pts_host if self._pts_host is not None else self._pts
        if src is None:
            return
        ok = bool(np.isfinite(src).all()) if isinstance(src, np.ndarray) else bool(torch.isfinite(src).all().item())
        if not ok:
            raise ValueError(f"{what}: the cloud has non-finite coordinates")

    def remove_radius_outlier(self, nb_points: int, radius: float, print_progress: bool = False):
        """Open3D RemoveRadiusOutliers: keep the points with more than
        nb_points points within radius (d^2 < radius^2, the point itself
        counted; ops.radius_count, the sweep stops at nb_points + 1).
        Returns (cloud, kept index list), as remove_statistical_outlier."""
        radius = float(radius)
        if int(nb_points) < 1 or not np.isfinite(radius) or radius < 0.0:
            raise ValueError("Illegal input parameters, the number of points must be positive and the radius "
                             "finite and not negative.")
        self._require_finite_points("remove_radius_outlier")
        if not self.has_points():
            return self.__class__(), []
        cnt = ops.radius_count(self._hot_points(), radius, cap=int(nb_points) + 1)
        keep = torch.nonzero(cnt > int(nb_points)).reshape(-1)
        return self._select_by_idx(keep), keep.cpu().numpy().tolist()

    def get_index_by_iss_keypoints(self, salient_radius: float = 0.0, non_max_radius: float = 0.0,
                                   gamma_21: float = 0.975, gamma_32: float = 0.975, min_neighbors: int = 5):
        """The ISS keypoints (o3d.geometry.keypoint.compute_iss_keypoints) as
        ascending int64 numpy indices (ops.iss_keypoints; Open3D's order is
        arbitrary).  Radii of 0.0: 6 and 4 model resolutions."""
        for name, v in (("salient_radius", salient_radius), ("non_max_radius", non_max_radius)):
            if not np.isfinite(float(v)) or float(v) < 0.0:
                raise ValueError(f"{name} must be finite and >= 0, got {v}")
        for name, v in (("gamma_21", gamma_21), ("gamma_32", gamma_32)):
            if not np.isfinite(float(v)):
                raise ValueError(f"{name} must be finite, got {v}")
        self._require_finite_points("compute_iss_keypoints")
        if not self.has_points():
            return np.zeros(0, np.int64)
        idx, _, _ = ops.iss_keypoints(self._hot_points(), float(salient_radius), float(non_max_radius),
                                      float(gamma_21), float(gamma_32), int(min_neighbors))
        return idx.cpu().numpy().astype(np.int64)

    def compute_iss_keypoints(self, salient_radius: float = 0.0, non_max_radius: float = 0.0,
                              gamma_21: float = 0.975, gamma_32: float = 0.975, min_neighbors: int = 5):
        """A new cloud of the ISS keypoints, every attribute following
        (get_index_by_iss_keypoints, _select_by_idx)."""
        idx = self.get_index_by_iss_keypoints(salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors)
        if not self.has_points():
            return self.__class__()
        return self._select_by_idx(idx)

    def merge_pcds(self, raw_pcds, rgb: bool = False, intensity: bool = False, normals: bool = False,
                   labels: bool = False):
        pcds = [p if isinstance(p, PointCloudBase) else self.__class__(p) for p in raw_pcds]
        res = self.__class__(np.vstack([p.get_points() for p in pcds]))
        if rgb:
            res.set_rgb(np.vstack([p.get_colors() if p.has_colors() else np.ones((p.size(), 3)) for p in pcds]))
        if normals:
            for p in pcds:
                if not p.has_normals():
                    p.estimate_normals()
            res.set_normals(np.vstack([p.get_normals() for p in pcds]))
        if intensity:
            res.set_intensity(np.vstack([p.get_intensity() if p.has_intensity()
                                         else p.set_uniform_intensity(0).get_intensity() for p in pcds]))
        if labels:
            res.labels = np.vstack([p.get_labels() if p.has_labels() else p.set_uniform_label(0).get_labels()
                                    for p in pcds])
        return res

    def append_pcd(self, pcd, rgb=False, intensity=False, normals=False, labels=False):
        return self.merge_pcds([self, pcd], rgb=rgb, intensity=intensity, normals=normals, labels=labels)

    def distance2plane(self, plane) -> np.ndarray:
        """Signed float64 distance to the plane (reference PointCloud.py:400-404),
        computed on the GPU in numpy's order ((x*a + y*b) + z*c + d) / |abc|, on
        the caller's float64 coordinates when the cloud holds them."""
        if not self.has_points():
            return np.zeros(0)
        return ops.plane_distance(self._plane_points(), np.asarray(plane, np.float64).reshape(4)).cpu().numpy()

    def remove_plane_outlier(self, plane_model, thickness: float = 0.03, similarity: float = 0.999,
                             invert: bool = False):
        cand = self.get_index_by_normals_cosine(plane_model, similarity)
        sub = self._select_by_idx(cand)
        on = sub._plane_index_dev(plane_model, thickness).long()
        floor_idx = torch.as_tensor(np.asarray(cand, np.int64), device=on.device)[on]
        return self._select_by_idx(floor_idx), floor_idx.cpu().numpy()

    def project2plane(self, plane):
        plane = np.asarray(plane, np.float64)
        dis = self.distance2plane(plane).reshape(-1, 1) * plane[:3].reshape(1, 3)
        return self.__class__(self.get_points() - dis)

    def seg_plane_by_svd(self):
        p = self.get_points()
        c = p.mean(0)
        _, _, v = np.linalg.svd(p - c)
        a, b, cc = v[-1]
        return a, b, cc, -float((c * v[-1]).sum())


class PointCloudAdvanceIO(PointCloudUtility):
    """LAS I/O (reference PointCloud.py:496-567, 705-710) without laspy:
    las_io.py holds the format rules; with a GPU the records are decoded and
    encoded by o3dx_las_unpack / o3dx_las_pack, without one by the numpy forms
    of the same rules (identical values).  get_lasdata is not mirrored: it
    returns laspy objects.  E57 I/O (reference PointCloud.py:569-703) without
    pye57: e57_io.py holds the format rules and the E57File object; with a GPU
    the page checksums, the record decode and the encode run in
    o3dx_e57_crc_pages / o3dx_e57_unpack / o3dx_e57_pack / o3dx_e57_seal,
    without one in the numpy forms (identical values).  Compressed LAZ, E57
    spherical coordinates and images2D, and the image I/O are out of scope."""

    def get_lasdata(self, *args, **kwargs):
        """Not mirrored: the reference returns a laspy.LasData (PointCloud.py:
        499-521), and this package has no laspy.  save_las / append_save_las
        fill the records by the same rules."""
        raise NotImplementedError("get_lasdata returns laspy objects and is not mirrored; use save_las / "
                                  "append_save_las")

    def _las_cloud(self, raw: np.ndarray, h, rgb: bool, intensity: bool, labels: bool):
        """A new cloud from a block of LAS records."""
        c = self.__class__()
        if raw.size == 0:
            return c
        if torch.cuda.is_available():
            d = las_io.decode_device(raw, h, _device(), rgb, intensity, labels)
            # the kernel's flag makes _wide known without set_points' passes; a
            # wide cloud keeps its float64 device copy, as set_points' torch branch
            c._pts = d["points32"]
            c._wide = d["wide"]
            c._pts64 = d["points64"]
            if rgb:
                c._colors = d["rgb"]
        else:
            d = las_io.decode_host(raw, h, rgb, intensity, labels)
            c.set_points(d["points"])
            if rgb:
                c.set_rgb(d["rgb"])
        if intensity:
            c.set_intensity(d["intensity"])
        if labels:
            c.set_labels(d["labels"])
        return c

    @staticmethod
    def _las_header(path: str, rgb: bool):
        h = las_io.read_header(path)
        if rgb and not h.has_rgb:
            raise ValueError(f"{path}: point format {h.point_format} has no colour (rgb=True)")
        return h

    def read_las(self, path: str, rgb: bool = False, intensity: bool = False, labels: bool = False):
        """A new cloud from a LAS 1.0-1.4 file, point formats 0-10,
        uncompressed (reference PointCloud.py:523-533).  Points are the
        float64 X * scale + offset; such values are rarely float32 values, so
        the cloud usually runs the float64 kernels (_wide).  rgb: colours
        u16 / 65536 (ValueError when the format has none); intensity: (n,1)
        uint16; labels: (n,1) uint8, the whole classification byte — laspy's
        raw_classification for formats 0-5, byte 16 for formats 6+ (this
        project's rule: laspy has no raw_classification there).  With a GPU
        the file's records go to the device once and are decoded there.
        RuntimeError names the file and the reason for a bad signature, an
        unknown or compressed (LAZ) point format, a record length below the
        format's minimum and truncated point data."""
        h = self._las_header(path, rgb)
        return self._las_cloud(las_io.read_records(h), h, rgb, intensity, labels)

    def read_las_gen(self, path: str, every_k_points: int = 100_0000, rgb: bool = False, intensity: bool = False,
                     labels: bool = False):
        """read_las in chunks (reference PointCloud.py:535-547): a generator of
        clouds of at most every_k_points consecutive records, each read from
        the file and decoded on its own; the file is never resident at once."""
        k = int(every_k_points)
        if k < 1:
            raise ValueError(f"every_k_points must be >= 1, got {every_k_points}")
        h = self._las_header(path, rgb)
        count = 0
        while count < h.count:
            m = min(k, h.count - count)
            pcd = self._las_cloud(las_io.read_records(h, count, m), h, rgb, intensity, labels)
            count += m
            print(f"[read_las_gen]: read {count / h.count * 100}% points.")
            yield pcd

    def _las_records(self, what: str, point_format: int, stride: int, scales, offsets, float32_coords: bool):
        """(records (n, stride) uint8 numpy, stats) of this cloud; raises before
        anything is written."""
        if self.has_rgb() and las_io.LAYOUT[point_format][2] is None:
            raise ValueError(f"{what}: the cloud has colours and point format {point_format} has none")
        # the reference's conversions (get_lasdata, PointCloud.py:511-512, 519-520), on the host
        inten = cls = None
        if self.has_intensity():
            inten = (np.asarray(self.get_intensity()).flatten() * 255).astype(np.uint8).astype(np.uint16)
        if self.has_labels():
            cls = np.asarray(self.labels).flatten().astype(np.uint8)
        if torch.cuda.is_available():
            dev = _device()
            x = self._dev_points() if float32_coords else self._hot_points()
            up = lambda a: None if a is None else torch.from_numpy(a).to(dev)  # noqa: E731
            rec, stats = ops.las_pack(x, stride, point_format, scales, offsets,
                                      rgb=self._colors.to(dev) if self.has_rgb() else None,
                                      intensity=up(None if inten is None else inten.view(np.int16)), labels=up(cls))
            stats = stats.cpu().numpy()
            las_io.check_stats(stats, what)
            return rec.cpu().numpy(), stats
        pts = self._dev_points().numpy() if float32_coords else self.get_points()
        rec, stats = las_io.pack_host(pts, point_format, stride, scales, offsets,
                                      rgb=self._colors.numpy() if self.has_rgb() else None, intensity=inten,
                                      labels=cls)
        las_io.check_stats(stats, what)
        return rec, stats

    def save_las(self, path: str = './pcd.las', pt_src_id: bool = False, *, scales=None, offsets=None,
                 point_format: int = 3, float32_coords: bool = True):
        """Write the cloud as LAS 1.2 (reference PointCloud.py:560-565).  The
        defaults reproduce the reference: point format 3, scales 1e-4, offsets
        0, coordinates cast to float32 first (get_lasdata's
        ps[:, 0].astype(np.float32)).  float32_coords=False quantises the
        cloud's float64 values directly, so a georeferenced cloud can be
        written with suitable offsets.  X = np.round((x - offset) / scale).
        Colours are written as (uint8)(c * 255) into the u16 fields and
        intensity as (uint8)(i * 255), the reference's conversions: read_las
        returns such a colour 256-fold dimmed (c * 255 / 65536), and an
        intensity i as int(i * 255) mod 256.  point_format: 0-3 or 6-8.
        OverflowError when a scaled coordinate leaves int32 (as laspy),
        ValueError for non-finite coordinates (this project's rule); in both
        cases nothing is written.  pt_src_id=True (the reference's per-scan
        source id of a stacked E57 cloud) is not mirrored:
        NotImplementedError."""
        if pt_src_id:
            raise NotImplementedError("save_las(pt_src_id=True): the per-scan point source id is not mirrored")
        if point_format not in las_io.WRITABLE:
            raise ValueError(f"save_las: point format {point_format} cannot be written (only {las_io.WRITABLE})")
        sc = np.full(3, 1e-4) if scales is None else np.broadcast_to(np.asarray(scales, np.float64), (3,)).copy()
        of = np.zeros(3) if offsets is None else np.broadcast_to(np.asarray(offsets, np.float64), (3,)).copy()
        if not (np.isfinite(sc).all() and (sc != 0).all() and np.isfinite(of).all()):
            raise ValueError("save_las: scales must be finite and non-zero, offsets finite")
        stride = las_io.LAYOUT[point_format][0]
        rec, stats = self._las_records(f"save_las({path})", point_format, stride, sc, of, float32_coords)
        las_io.write_file(path, las_io.build_header(point_format, stride, len(rec), sc, of, stats), rec)

    def append_save_las(self, path: str = './pcd.las', pt_src_id: bool = False):
        """Append the cloud to an existing LAS file (reference PointCloud.py:
        549-558) with that file's point format, record length, scales and
        offsets; the point count (legacy, and the u64 count of LAS 1.4) and the
        merged min / max are rewritten.  AssertionError when the file does not
        exist; RuntimeError when bytes follow the point block (EVLRs) or the
        format is not one save_las writes; on OverflowError / ValueError the
        file is left as it was."""
        assert os.path.isfile(path), f'file {path} is no exist.'
        if pt_src_id:
            raise NotImplementedError("append_save_las(pt_src_id=True): the per-scan point source id is not mirrored")
        h = las_io.read_header(path)
        las_io.check_appendable(h)
        rec, stats = self._las_records(f"append_save_las({path})", h.point_format, h.stride, h.scales, h.offsets, True)
        las_io.append_records(h, rec, stats)

    def pcd2las(self, from_path: str, to_path: str = None):
        """The reference's two-step converter (PointCloud.py:705-710): a
        generator yielding 0.5 after reading the PCD and 1.0 after save_las."""
        if to_path is None:
            to_path = from_path.replace('.pcd', '.las')
        p = self.read_pcd(from_path)
        yield 0.5
        p.save_las(to_path)
        yield 1.0

    # ------------------------------------------------------------------ E57
    def _e57_open(self, file_path: str, rgb: bool, intensity: bool, row_column: bool):
        """The cloud's E57File, opened on first use and re-used after (as the
        reference: PointCloud.py:637-643), with the switches of this call."""
        if self.e57 is None:
            self.e57 = e57_io.E57File(file_path, intensity=intensity, colors=rgb, row_column=row_column,
                                      printinfo=True)
        else:
            self.e57.intensity = intensity
            self.e57.colors = rgb
            self.e57.row_column = row_column
            self.e57.point_file = file_path
        return self.e57

    def _e57_cloud(self, parts, scan_No: int):
        """A new cloud from decoded E57 records (E57File.decode dicts, stacked)."""
        c = self.__class__()
        c.e57 = self.e57
        c.scan_No = scan_No
        parts = [d for d in parts if len(d["points32"] if d["device"] else d["points"])]
        if not parts:
            return c
        dev = parts[0]["device"]
        cat = (lambda a: a[0] if len(a) == 1 else torch.cat(a)) if dev else \
            (lambda a: a[0] if len(a) == 1 else np.concatenate(a))
        col = lambda k: None if parts[0][k] is None else cat([d[k] for d in parts])  # noqa: E731
        rgb, inten, row, column = col("rgb"), col("intensity"), col("row"), col("col")
        if dev:
            # the kernel's flag makes _wide known without set_points' passes, as _las_cloud
            c._pts = cat([d["points32"] for d in parts])
            c._wide = any(d["wide"] for d in parts)
            c._pts64 = cat([d["points64"] for d in parts]) if c._wide else None
            if rgb is not None:
                # the constructor's rule (reference PointCloud.py:36-40) in float64, on the device
                r = rgb.double()
                if float(r.max()) > 1.0:
                    r = (r - r.min()) / (r.max() - r.min())
                c._colors = r.float().contiguous()
            inten, row, column = (None if t is None else t.cpu().numpy() for t in (inten, row, column))
            if row is not None:
                row, column = row.view(np.uint16), column.view(np.uint16)
        else:
            c.set_points(cat([d["points"] for d in parts]))
            if rgb is not None:
                c._set_rgb_rescaled(rgb)
        if inten is not None:
            c.set_intensity(np.expand_dims(inten, 1))
        if row is not None:
            c.row_index, c.column_index = row, column
        return c

    def read_e57(self, file_path: str, scan_No: int = -1, rgb: bool = False, intensity: bool = False,
                 row_column: bool = False, infoOnly: bool = False):
        """A new cloud from an E57 file (reference PointCloud.py:627-644)
        without pye57: scan scan_No, or all scans stacked for -1.  As pye57's
        read_scan, rows whose cartesianInvalidState is not 0 are dropped and
        the scan's pose transforms the points (R from the quaternion, x' =
        ((R00 x + R01 y) + R02 z) + t0 in float64: this project's rule).
        Cartesian coordinates stored as Float single give a float32 cloud;
        Float double and ScaledInteger scans usually run the float64 kernels
        (_wide).  rgb: the Integer colours through the constructor's rule
        (values above 1 are min-max rescaled); intensity: (n,1) float32;
        row_column: uint16 row_index / column_index.  ValueError when a field
        asked for is missing.  The result carries .e57 (the E57File) and
        .scan_No; infoOnly returns an empty cloud with .e57 set.  With a GPU
        the file's bytes go to the device once: the page checksums and the
        decode run there.  RuntimeError names the file and the reason for a
        bad signature, major version or page size, a length that is no
        multiple of the page size, truncated data, a CRC mismatch (with the
        first bad page), a stream too short for recordCount and spherical-only
        scans."""
        e = self._e57_open(file_path, rgb, intensity, row_column)
        if infoOnly:
            c = self.__class__()
            c.e57 = e
            return c
        scans = range(e.scan_count) if scan_No < 0 else [scan_No]
        return self._e57_cloud([e.decode(i, 0, e.scan_headers[i].point_count, local=False) for i in scans], scan_No)

    def read_e57_gen(self, file_path: str, rgb: bool = False, intensity: bool = False, row_column: bool = False):
        """read_e57 scan by scan (reference PointCloud.py:646-656)."""
        e = self._e57_open(file_path, rgb, intensity, row_column)
        for i in range(e.scan_count):
            yield self._e57_cloud([e.decode(i, 0, e.scan_headers[i].point_count, local=False)], i)

    def read_e57_scan_gen(self, file_path: str, scan_No: int = 0, rgb: bool = False, intensity: bool = False,
                          row_column: bool = False, every_k_points: int = 10000000):
        """One scan in chunks of every_k_points records (reference
        PointCloud.py:658-671).  The chunks hold the scan's raw local
        coordinates, unfiltered: no pose, invalid rows kept, as the
        reference's raw-buffer path yields them.  Exactly ceil(count /
        every_k_points) chunks: the reference's extra stale chunk at exact
        multiples is not mirrored."""
        e = self._e57_open(file_path, rgb, intensity, row_column)
        for r0, m in e.chunks(scan_No, every_k_points):
            yield self._e57_cloud([e.decode(scan_No, r0, m, local=True)], scan_No)

    def read_e57_gen_scan_gen(self, file_path: str, rgb: bool = False, intensity: bool = False,
                              row_column: bool = False, every_k_points: int = 10000000):
        """read_e57_scan_gen over every scan (reference PointCloud.py:673-687):
        raw local coordinates, unfiltered, ceil(count / every_k_points) chunks
        per scan."""
        e = self._e57_open(file_path, rgb, intensity, row_column)
        for i in range(e.scan_count):
            for r0, m in e.chunks(i, every_k_points):
                yield self._e57_cloud([e.decode(i, r0, m, local=True)], i)

    def _e57_scan(self, normals: bool):
        """(ScanPlan, XML kinds, columns, bounds, intensity limits) of this
        cloud as one written scan.  Columns are (tensor, stride, first) on the
        device, 1-d numpy arrays without one."""
        S = e57_io
        n = self.size()
        gpu = torch.cuda.is_available()
        fields, kinds, cols = [], [], []

        def add(name, src, bits, kind, col, mn=0, mx=0):
            fields.append((name, src, bits, mn, mx))
            kinds.append(kind)
            cols.append(col)

        def split3(t, names, src, bits, kind):
            for a, nm in enumerate(names):
                add(nm, src, bits, kind, (t, 3, a) if gpu else np.ascontiguousarray(t[:, a]))

        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(_device())  # noqa: E731
        xyz_names = ("cartesianX", "cartesianY", "cartesianZ")
        if self._wide:
            p = self._hot_points() if gpu else self.get_points()
            split3(p, xyz_names, S.SRC_F64, 64, "double")
        else:
            p = self._dev_points() if gpu else self._dev_points().numpy()
            split3(p, xyz_names, S.SRC_F32, 32, "single")
        bounds = limits = None
        if n:
            lo, hi = (p.amin(0), p.amax(0)) if gpu else (p.min(0), p.max(0))
            lo, hi = _as_np(lo).astype(np.float64), _as_np(hi).astype(np.float64)
            bounds = [lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]]
        if self.has_intensity():
            i32 = np.asarray(self.get_intensity()).flatten().astype(np.float32)
            limits = (float(i32.min()), float(i32.max()))
            add("intensity", S.SRC_F32, 32, "single", (up(i32), 1, 0) if gpu else i32)
        if self.has_rgb():
            c = self._colors.to(_device()) if gpu else self._colors.cpu().numpy()
            split3(c, ("colorRed", "colorGreen", "colorBlue"), S.SRC_COLOUR, 8, (0, 255))
        if self.has_col_row():
            column, row = self.get_col_row()
            for nm, v in (("rowIndex", row), ("columnIndex", column)):
                v = np.asarray(v).flatten().astype(np.int64)
                if v.min() < 0:
                    raise ValueError(f"save_e57: {nm} has negative values")
                mx = int(v.max())
                add(nm, S.SRC_I64, mx.bit_length(), (0, mx), (up(v), 1, 0) if gpu else v, 0, mx)
        if normals and self.has_normals():
            nr = self._normals.to(_device()) if gpu else self._normals.cpu().numpy()
            split3(nr, ("nor:normalX", "nor:normalY", "nor:normalZ"), S.SRC_F32, 32, "single")
        return S.ScanPlan(fields, n), kinds, cols, bounds, limits

    @staticmethod
    def _e57_write(filename: str, clouds, name, rotation, translation, normals: bool):
        S = e57_io
        scans = [c._e57_scan(normals) for c in clouds]
        plans = [s[0] for s in scans]
        secs, xml_at = S.layout(plans)
        parts = [S.scan_xml(p, S.physical(sec), name or f"scan {i}", f"{{{uuid.uuid4()}}}", s[3], s[4], rotation,
                            translation, s[1]) for i, (p, sec, s) in enumerate(zip(plans, secs, scans))]
        xml = S.file_xml(parts, any(f[0].startswith("nor:") for p in plans for f in p.fields))
        size = (xml_at + len(xml) + 3) // 4 * 4
        head = np.frombuffer(S.file_header(xml_at, len(xml)), np.uint8)
        gpu = torch.cuda.is_available()
        image = torch.zeros(size, dtype=torch.uint8, device=_device()) if gpu else np.zeros(size, np.uint8)
        put = (lambda at, b: image[at:at + len(b)].copy_(torch.from_numpy(np.array(b)))) if gpu else \
            (lambda at, b: image.__setitem__(slice(at, at + len(b)), b))
        put(0, head)
        put(xml_at, np.frombuffer(xml, np.uint8))
        for p, sec, s in zip(plans, secs, scans):
            put(sec, np.frombuffer(S.section_header(p, sec), np.uint8))
            if not p.packets:
                continue
            at = sec + S.SECTION_HEADER
            if gpu:
                ops.e57_pack(p.tables(), s[2], p.n, p.R, p.full_bytes, p.last_bytes, p.packet_head(False),
                             p.packet_head(True), out=image[at:at + p.data_bytes])
            else:
                image[at:at + p.data_bytes] = S.pack_host(p, s[2])
        paged = ops.e57_seal(image).cpu().numpy() if gpu else S.seal_host(image)
        paged.tofile(filename)

    def save_e57(self, filename: str, name: str = None, rotation: np.ndarray = None, translation: np.ndarray = None,
                 labels: bool = False, normals: bool = True):
        """Write the cloud as a one-scan E57 file (reference PointCloud.py:
        614-625) without pye57.  cartesianX/Y/Z are Float double when the
        cloud holds float64 values float32 cannot (_wide), else Float single;
        intensity Float single with intensityLimits; colours Integer 0..255,
        (uint8)(c * 255) as the reference's _get_data_raw_e57; rowIndex /
        columnIndex Integer 0..max; the stored normals as nor:normalX/Y/Z Float
        single (normals=False leaves them out).  rotation (quaternion w, x, y,
        z) / translation are written as the scan's pose: read_e57 applies
        them.  labels is accepted and unused, as in the reference.  Packets
        hold a fixed number of records (the largest multiple of 8 that keeps a
        packet within 65,536 bytes); no index packet is written.  With a GPU
        the packets and the page checksums are built there."""
        self._e57_write(filename, [self], name, rotation, translation, normals)

    def save_pcds_e57(self, pcds, filename: str, name: str = None, rotation: np.ndarray = None,
                      translation: np.ndarray = None, labels: bool = False):
        """One E57 file with one scan per cloud of pcds (reference
        PointCloud.py:600-612, which writes this cloud's data once per entry;
        here every entry's own data), without normals."""
        self._e57_write(filename, list(pcds), name, rotation, translation, False)

    def e572las(self, from_path: str, to_path: str = None, rgb: bool = False, intensity: bool = False,
                row_column: bool = False, every_k_points: int = 10000000):
        """E57 to LAS in chunks (reference PointCloud.py:689-703): a generator
        of progress fractions; the first chunk goes through save_las, the rest
        through append_save_las (raw local coordinates, as read_e57_gen_scan_gen
        yields them)."""
        if to_path is None:
            to_path = from_path.replace('.e57', '.las')
        cnt = 0
        for i, p in enumerate(self.read_e57_gen_scan_gen(from_path, rgb, intensity, row_column, every_k_points)):
            p.save_las(to_path) if i == 0 else p.append_save_las(to_path)
            cnt += p.size()
            del p
            yield cnt / self.e57.all_points


class PointCloud(PointCloudAdvanceIO):

    def split_pcd_index(self, nn: int, random: bool = False):
        n = self.size()
        if n <= nn:
            return [np.arange(n)]
        parts = n // nn
        sizes = np.full(parts, nn) + np.asarray([len(a) for a in np.array_split(np.ones(n % nn), parts)])
        r = np.arange(n)
        if random:
            np.random.shuffle(r)
        starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
        return [r[s:s + k] for s, k in zip(starts, sizes)]

    def split_pcd(self, nn: int, random: bool = False):
        if self.size() <= nn:
            return [self]
        return [self._select_by_idx(i) for i in self.split_pcd_index(nn=nn, random=random)]

    def split_by_voxel(self, voxel_size: float = 0.01, random: bool = True, top_n: int = 10):
        """Round-robin one point per voxel into up to top_n clouds (reference
        PointCloud.py:735-757), using the GPU voxel trace."""
        lists = [np.asarray(v).tolist() for v in self.voxel_down_sample_and_trace(voxel_size)[2]]
        if random:
            for v in lists:
                np.random.shuffle(v)
        pcds, taken = [], []
        while True:
            pick = [v.pop() for v in lists if len(v) > 0]
            if not pick:
                break
            taken += pick
            pcds.append(self._select_by_idx(pick))
            if len(pcds) >= top_n:
                break
        return pcds, self._select_by_idx(taken, True)

    def rotation_matrix_from_vectors(self, vec1, vec2) -> np.ndarray:
        a = (np.asarray(vec1, np.float64) / np.linalg.norm(vec1)).reshape(3)
        b = (np.asarray(vec2, np.float64) / np.linalg.norm(vec2)).reshape(3)
        v = np.cross(a, b)
        if not any(v):
            return np.eye(3)
        c = np.dot(a, b)
        s = np.linalg.norm(v)
        K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
        return np.eye(3) + K + K @ K * ((1 - c) / s ** 2)

    def rotate_by_normal(self, plane):
        a, b, c, d = plane
        T = np.eye(4)
        T[2, 3] = d
        T[:3, :3] = self.rotation_matrix_from_vectors(np.array([a, b, c]) / np.linalg.norm([a, b, c]), (0, 0, 1))
        self.transform(T)
        return self, T

    rotate_to_plane = rotate_by_normal

    def seg_planes(self, thickness: float = 0.01, ransac_n: int = 3, num_iterations: int = 450,
                   top_n: float = 10e9, minPointsRatio: float = 0.1):
        """Repeated GPU segment_plane on the remaining outliers (reference
        PointCloud.py:941-985) -> (planes, pcds (inliers..., outliers), aabbs)."""
        rest, planes, pcds, aabbs = self, [], [], []
        raw = self.size()
        if raw < ransac_n:
            return planes, pcds, aabbs
        while rest.size() / raw > minPointsRatio:
            try:
                # the inliers stay on the device between the rounds
                plane, inl = rest._segment_plane_dev(thickness, ransac_n, num_iterations)
            except RuntimeError as e:
                print(e)
                break
            if inl.numel() == 0:
                # every hypothesis degenerate (a collinear or coincident
                # remainder): the zero plane, and `rest` cannot change
                break
            planes.append(plane)
            inliers = rest._select_by_idx(inl)
            pcds.append(inliers)
            aabbs.append(inliers.get_aabb())
            rest = rest._select_by_idx(inl, True)
            if len(planes) > top_n:
                break
        pcds.append(rest)
        aabbs.append(rest.get_aabb())
        return planes, pcds, aabbs

    def DBSCAN(self, eps: float = 0.05, min_samples: int = 3):
        """sklearn.cluster.DBSCAN(eps, min_samples).fit(get_points()) on the GPU
        (reference PointCloud.py:921-927) -> ([cloud per cluster], labels).
        labels: sklearn's labels_ (int64 numpy; clusters numbered by ascending
        smallest core index, noise -1); cluster i is _select_by_idx of the
        ascending indices with label i, every attribute carried.  ValueError,
        as sklearn raises, for eps <= 0, min_samples < 1, an empty cloud or
        non-finite coordinates.  sklearn's other arguments (metric,
        sample_weight, n_jobs) are not offered."""
        eps = float(eps)
        if not (eps > 0.0) or not np.isfinite(eps):
            raise ValueError(f"eps must be a finite float > 0, got {eps}")
        if int(min_samples) != min_samples or int(min_samples) < 1:
            raise ValueError(f"min_samples must be an int >= 1, got {min_samples}")
        if not self.has_points():
            raise ValueError("Found array with 0 sample(s) (shape=(0, 3)) while a minimum of 1 is required by DBSCAN.")
        if self._pts_host is not None:
            finite = bool(np.isfinite(self._pts_host).all())
        else:
            src = self._pts64 if self._pts64 is not None else self._pts
            finite = bool(torch.isfinite(src).all().item())
        if not finite:
            raise ValueError("Input contains NaN or infinity.")
        lab, k = ops.dbscan(self._hot_points(), eps, int(min_samples))
        # one stable sort groups the indices by label, ascending inside each
        order = torch.sort(lab, stable=True).indices
        counts = torch.bincount((lab + 1).long(), minlength=k + 1).cpu().numpy()
        ends = np.cumsum(counts)  # label -1 first
        pcds = [self._select_by_idx(order[ends[i]:ends[i + 1]]) for i in range(k)]
        return pcds, lab.cpu().numpy().astype(np.int64)

    # ------------------------------------------------ floor-map segmentation
    def _finite_points(self) -> bool:
        if self._pts_host is not None:
            return bool(np.isfinite(self._pts_host).all())
        src = self._pts64 if self._pts64 is not None else self._pts
        return bool(torch.isfinite(src).all().item())

    def _raster(self, resolution: float, want_winner: bool = False):
        """ops.raster2d of this cloud's get_points() values (the float64 host
        values when the cloud holds them, else the float32 points)."""
        resolution = float(resolution)
        if not (resolution > 0.0) or not np.isfinite(resolution):
            raise ValueError(f"resolution must be a finite float > 0, got {resolution}")
        if not self.has_points():
            raise ValueError("to_2D_Img: the cloud has no points")
        if not self._finite_points():
            raise ValueError("to_2D_Img: the coordinates must be finite")
        return ops.raster2d(self._plane_points(), resolution, want_winner=want_winner)

    def to_2D_Img(self, resolution: float = 0.05, color: bool = False):
        """The cloud's (x, y) rasterised at `resolution` on the GPU (reference
        PointCloud.py:785-823; include/o3dx.h states the rule) ->
        (img, minx, T, miny, invT, resolution, idx2img).  img: (sizey, sizex)
        uint8, 255 on every hit pixel; with color=True and colours present
        (sizey, sizex, 3) uint8, the colour (get_colors() * 255 as uint8) of
        the highest point index on each pixel (numpy's last write wins).  T
        maps the points to pixel coordinates, invT = inv(T).  idx2img is an
        (N,2) int64 numpy array of (ix, iy) where the reference returns a
        Python list of N tuples: every consumer does np.asarray(idx2img), for
        which the array is identical.  ValueError for a resolution <= 0 or not
        finite, an empty cloud or non-finite coordinates (the reference's
        result there is garbage); IndexError when all points fall in one pixel
        column or row, as the reference's indexing raises."""
        usecolor = bool(color) and self.has_colors()
        if color and not usecolor:
            print('has no rgb data, cannot use color!')
        r = self._raster(resolution, want_winner=usecolor)
        minx, miny = r["minx"], r["miny"]
        T = np.asarray([[1., 0., 0., -minx],
                        [0., 1., 0., -miny],
                        [0., 0., 1., 0.],
                        [0., 0., 0., 1.]])
        ir = 1 / resolution
        T = np.asarray([[ir, 0., 0., 0.],
                        [0., ir, 0., 0.],
                        [0., 0., ir, 0.],
                        [0., 0., 0., 1.]]) @ T
        if usecolor:
            win = r["winner"].cpu().numpy()
            rgb = (self.get_colors() * 255).astype(np.uint8)
            img = np.zeros((r["h"], r["w"], 3), np.uint8)
            hit = win >= 0
            img[hit] = rgb[win[hit]]
        else:
            img = r["img"].cpu().numpy()
        idx2img = r["pix"].cpu().numpy().astype(np.int64)
        return img, minx, T, miny, np.linalg.inv(T), resolution, idx2img

    @staticmethod
    def _ccl_ranking(areas: np.ndarray) -> np.ndarray:
        """The labels the segmentation returns, in order: all labels (the
        background included) ranked by area, descending — equal areas with the
        higher label first (this project's rule; the reference's unstable
        argsort leaves ties open) — without the first of that ranking,
        whichever label it is (reference PointCloud.py:894, 910)."""
        return np.argsort(np.asarray(areas), kind="stable")[::-1][1:]

    def _ccl_clouds(self, img_dev: torch.Tensor, pix_dev: torch.Tensor, top_n=None, minpoints: int = 0):
        labels, areas, k = ops.ccl2d(img_dev)
        _, order, counts = ops.label_group(pix_dev, labels, k)
        counts = counts.cpu().numpy()
        ends = np.concatenate([[0], np.cumsum(counts)])
        rank = self._ccl_ranking(areas.cpu().numpy())
        if top_n is not None:
            rank = rank[:max(int(top_n), 0)]
        pcds = []
        for l in rank:
            if counts[l] < minpoints:
                continue
            pcds.append(self._select_by_idx(order[ends[l]:ends[l + 1]]))
        return pcds

    def simple_seg_connected_components_by_img(self, img: np.ndarray, minx=None, T=None, miny=None, invT=None,
                                               resolution=None, idx2img=None):
        """One cloud per 8-connected component of the 2-D uint8 image `img`
        (non-zero = foreground), labelled on the GPU: the points whose pixel
        idx2img[i] = (ix, iy) carries the component's label, for every label of
        _ccl_ranking (no top_n, no minpoints: empty clouds are included)
        (reference PointCloud.py:888-897; the arguments are to_2D_Img's
        tuple).  IndexError when len(idx2img) != size() or an index lies
        outside the image — a negative one too, where numpy would wrap."""
        im = _as_np(img)
        if im.ndim != 2:
            raise ValueError(f"img must be a 2-D image, got shape {im.shape}")
        if im.dtype != np.uint8:
            im = (im != 0).astype(np.uint8)
        idx = np.asarray(idx2img)
        if idx.ndim != 2 or idx.shape[1] != 2 or len(idx) != self.size():
            raise IndexError(f"idx2img must hold one (ix, iy) per point: shape {idx.shape} for {self.size()} points")
        if len(idx) == 0 or im.size == 0:
            raise IndexError("simple_seg_connected_components_by_img: no points or an empty image")
        h, w = im.shape
        if idx.min() < 0 or idx[:, 0].max() >= w or idx[:, 1].max() >= h:
            raise IndexError(f"idx2img has an index outside the {h} x {w} image")
        dev = N.default_device()
        img_dev = torch.as_tensor(np.ascontiguousarray(im), device=dev)
        pix_dev = torch.as_tensor(np.ascontiguousarray(idx, dtype=np.int32), device=dev)
        return self._ccl_clouds(img_dev, pix_dev)

    def simple_seg_connected_components(self, plane, thickness: float = 0.05, resolution: float = 0.1,
                                        minpoints: int = 20, top_n: int = 100):
        """The reference's floor-map segmentation (PointCloud.py:899-916) on
        the GPU: the slab within `thickness` of `plane`, rasterised at
        `resolution`, its 8-connected blobs labelled; the next top_n labels of
        _ccl_ranking each give the slab's points on that blob (ascending, all
        attributes carried), skipped below minpoints.  [] for an empty slab."""
        slab = self._select_by_idx(self._plane_index_dev(plane, thickness))
        if slab.size() == 0:
            return []
        r = slab._raster(resolution)
        return slab._ccl_clouds(r["img"], r["pix"], top_n=top_n, minpoints=minpoints)

    def registration_icp(self, target: "PointCloudBase", max_correspondence_distance: float, init=None,
                         max_iteration: int = 30, relative_fitness: float = 1e-6, relative_rmse: float = 1e-6,
                         estimation="point_to_plane"):
        """ICP of self onto target (Open3D registration_icp), on the GPU.
        estimation: "point_to_plane" (TransformationEstimationPointToPlane; the
        target needs normals) or "point_to_point"
        (TransformationEstimationPointToPoint, Umeyama; no normals needed), or
        one of the params.TransformationEstimation* objects (PointToPoint's
        with_scaling included).  NOTE: the default here is point-to-plane,
        where Open3D's registration_icp defaults to point-to-point — pass the
        estimation explicitly when porting a call that relies on Open3D's
        default.  ValueError on any other estimation.  North-star op; the
        reference has no ICP."""
        est, with_scaling = resolve_estimation(estimation)
        if est == "point_to_plane" and not target.has_normals():
            raise RuntimeError("TransformationEstimationPointToPlane and TransformationEstimationColoredICP "
                               "require pre-computed normal vectors for target PointCloud.")
        if max_correspondence_distance <= 0.0:
            raise RuntimeError("Invalid max_correspondence_distance.")
        wide = self._wide or target._wide
        src = self._plane_points() if wide else self._dev_points()
        tgt = target._plane_points() if wide else target._dev_points()
        if wide and est == "point_to_plane":
            _warn_offset_icp(self, target)
        r = ops.registration_icp(src, tgt, target._normals if target.has_normals() else None,
                                 max_correspondence_distance, init, max_iteration, relative_fitness, relative_rmse,
                                 estimation=est, with_scaling=with_scaling)
        return RegistrationResult(r["transformation"], r["fitness"], r["inlier_rmse"],
                                  r["correspondence_set"].cpu().numpy().astype(np.int64))

    # ------------------------------------------------- global registration
    def evaluate_registration(self, target: "PointCloudBase", max_correspondence_distance: float,
                              transformation=None):
        """Open3D evaluate_registration: fitness, inlier_rmse and the
        correspondences (every source point's nearest target point within the
        distance) under `transformation` — registration_icp at max_iteration=0."""
        return self.registration_icp(target, max_correspondence_distance, init=transformation, max_iteration=0,
                                     estimation="point_to_point")

    def compute_fpfh_feature(self, param=KDTreeSearchParamHybrid(0.1, 64)):
        """Open3D compute_fpfh_feature on the GPU -> params.Feature (.data (33,
        N) float64; the device rows are kept for the matcher).  The neighbour
        lists are this library's (sorted by (d^2, index), strict d^2 < r^2, the
        point itself included).  KNN(k) or Hybrid(radius, max_nn) with k,
        max_nn <= 64 (ValueError above); Radius raises NotImplementedError
        (unbounded lists); RuntimeError without normals, as Open3D; float64
        clouds that float32 cannot hold raise NotImplementedError."""
        mode, knn, radius = resolve(param)
        if mode == N.SEARCH_RADIUS:
            raise NotImplementedError("compute_fpfh_feature: KDTreeSearchParamRadius has unbounded neighbour lists; "
                                      "use KDTreeSearchParamHybrid(radius, max_nn <= 64) or KDTreeSearchParamKNN")
        if knn > N.MAX_KNN or knn < 1:
            raise ValueError(f"compute_fpfh_feature: knn / max_nn must be in 1..{N.MAX_KNN} (O3DX_MAX_KNN), got {knn}")
        if not self.has_normals():
            raise RuntimeError("Failed because input point cloud has no normal.")
        if self._wide:
            raise NotImplementedError("float64 clouds that float32 cannot hold are outside compute_fpfh_feature "
                                      "(pass float32 values)")
        return Feature(dev=ops.fpfh(self._dev_points(), self._normals, mode=mode, knn=knn, radius=radius))

    def _ransac_args(self, target, estimation, checkers, criteria, what):
        est, with_scaling = resolve_estimation(estimation)
        if est != "point_to_point" or with_scaling:
            raise ValueError(f"{what}: only TransformationEstimationPointToPoint(with_scaling=False) is supported")
        edge, dist = resolve_checkers(checkers)
        if self._wide or target._wide:
            raise NotImplementedError(f"float64 clouds that float32 cannot hold are outside {what} "
                                      "(pass float32 values)")
        return edge, dist, int(criteria.max_iteration), float(criteria.confidence)

    def registration_ransac_based_on_correspondence(self, target: "PointCloudBase", corres,
                                                    max_correspondence_distance: float,
                                                    estimation=TransformationEstimationPointToPoint(False),
                                                    ransac_n: int = 3, checkers=[],
                                                    criteria=RANSACConvergenceCriteria(100000, 0.999), seed=None):
        """Open3D registration_ransac_based_on_correspondence on the GPU
        (ops.registration_ransac_based_on_correspondence states the rule).
        corres: (C, 2) source / target indices.  The samples are
        ops.ransac_samples(C, ransac_n, max_iteration, seed) — distinct within
        a sample and seeded, where Open3D draws with replacement from an
        unseeded generator; seed=None takes the package's
        seed sequence (set_random_seed).  The result is the winning
        transformation evaluated over every source point, as Open3D returns
        it.  ransac_n < 3, fewer than ransac_n correspondences or a distance
        <= 0 give the empty result; ValueError for another estimation or the
        normal checker."""
        edge, dist, max_it, conf = self._ransac_args(target, estimation, checkers, criteria,
                                                     "registration_ransac_based_on_correspondence")
        c = corres if isinstance(corres, torch.Tensor) else np.asarray(corres).reshape(-1, 2)
        if ransac_n < 3 or len(c) < ransac_n or max_correspondence_distance <= 0.0:
            return RegistrationResult(np.eye(4), 0.0, 0.0, np.zeros((0, 2), np.int64))
        r = ops.registration_ransac_based_on_correspondence(
            self._dev_points(), target._dev_points(), c, max_correspondence_distance, ransac_n, edge, dist, max_it,
            conf, seed=_next_seed() if seed is None else seed)
        return self.evaluate_registration(target, max_correspondence_distance, r["transformation"])

    def registration_ransac_based_on_feature_matching(self, target: "PointCloudBase", source_feature, target_feature,
                                                      mutual_filter: bool, max_correspondence_distance: float,
                                                      estimation=TransformationEstimationPointToPoint(False),
                                                      ransac_n: int = 3, checkers=[],
                                                      criteria=RANSACConvergenceCriteria(100000, 0.999), seed=None):
        """Open3D registration_ransac_based_on_feature_matching on the GPU:
        the correspondences of ops.correspondences_from_features(source_feature,
        target_feature, mutual_filter), then
        registration_ransac_based_on_correspondence."""
        self._ransac_args(target, estimation, checkers, criteria, "registration_ransac_based_on_feature_matching")
        if ransac_n < 3 or max_correspondence_distance <= 0.0:
            return RegistrationResult(np.eye(4), 0.0, 0.0, np.zeros((0, 2), np.int64))
        if source_feature.num() != self.size() or target_feature.num() != target.size():
            raise RuntimeError("registration_ransac_based_on_feature_matching: one feature column per point")
        corres = ops.correspondences_from_features(source_feature.device_rows(), target_feature.device_rows(),
                                                   mutual_filter)
        return self.registration_ransac_based_on_correspondence(target, corres, max_correspondence_distance,
                                                                estimation, ransac_n, checkers, criteria, seed)
