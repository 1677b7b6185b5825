"""Search-parameter shims for estimate_normals / KD-tree queries.

The reference defaults to o3d.geometry.KDTreeSearchParamKNN(30)
(/root/reference/open3dpypro/PointCloud.py:68) and test_mesh.py:18 uses
KDTreeSearchParamHybrid(radius, max_nn).  Parameters are duck-typed on
.knn / .radius / .max_nn, so genuine open3d.geometry objects work too.
"""
from __future__ import annotations

from . import _native as N


class KDTreeSearchParamKNN:
    def __init__(self, knn: int = 30):
        self.knn = int(knn)

    def __repr__(self):
        return f"KDTreeSearchParamKNN(knn={self.knn})"


class KDTreeSearchParamRadius:
    def __init__(self, radius: float):
        self.radius = float(radius)

    def __repr__(self):
        return f"KDTreeSearchParamRadius(radius={self.radius})"


class KDTreeSearchParamHybrid:
    def __init__(self, radius: float, max_nn: int):
        self.radius = float(radius)
        self.max_nn = int(max_nn)

    def __repr__(self):
        return f"KDTreeSearchParamHybrid(radius={self.radius}, max_nn={self.max_nn})"


class TransformationEstimationPointToPoint:
    """Open3D's registration_icp default estimation (Umeyama; with_scaling
    also estimates a uniform scale)."""

    def __init__(self, with_scaling: bool = False):
        self.with_scaling = bool(with_scaling)

    def __repr__(self):
        return f"TransformationEstimationPointToPoint(with_scaling={self.with_scaling})"


class TransformationEstimationPointToPlane:
    def __repr__(self):
        return "TransformationEstimationPointToPlane()"


def resolve_estimation(estimation, with_scaling: bool = False):
    """-> (estimation name, with_scaling) of an estimation string or a
    TransformationEstimation object (duck-typed on the class name and
    .with_scaling, so genuine open3d.pipelines.registration objects work
    too).  ValueError on anything else."""
    if isinstance(estimation, str):
        if estimation not in N.ICP_ESTIMATIONS:
            raise ValueError(f"unknown ICP estimation {estimation!r}: one of {sorted(N.ICP_ESTIMATIONS)}")
        return estimation, bool(with_scaling) and estimation == "point_to_point"
    name = type(estimation).__name__
    if name == "TransformationEstimationPointToPoint":
        return "point_to_point", bool(getattr(estimation, "with_scaling", False))
    if name == "TransformationEstimationPointToPlane":
        return "point_to_plane", False
    raise ValueError(f"unsupported ICP estimation {estimation!r}: 'point_to_plane', 'point_to_point' or a "
                     "TransformationEstimationPointToPoint / TransformationEstimationPointToPlane object")


class RANSACConvergenceCriteria:
    """Open3D's criteria of the RANSAC registrations (max_iteration, confidence)."""

    def __init__(self, max_iteration: int = 100000, confidence: float = 0.999):
        self.max_iteration = int(max_iteration)
        self.confidence = float(confidence)

    def __repr__(self):
        return f"RANSACConvergenceCriteria(max_iteration={self.max_iteration}, confidence={self.confidence})"


class CorrespondenceCheckerBasedOnEdgeLength:
    def __init__(self, similarity_threshold: float = 0.9):
        self.similarity_threshold = float(similarity_threshold)

    def __repr__(self):
        return f"CorrespondenceCheckerBasedOnEdgeLength(similarity_threshold={self.similarity_threshold})"


class CorrespondenceCheckerBasedOnDistance:
    def __init__(self, distance_threshold: float):
        self.distance_threshold = float(distance_threshold)

    def __repr__(self):
        return f"CorrespondenceCheckerBasedOnDistance(distance_threshold={self.distance_threshold})"


def resolve_checkers(checkers):
    """-> (edge similarity, distance threshold) of a list of correspondence
    checkers, -1.0 where there is none (duck-typed on similarity_threshold /
    distance_threshold, so genuine Open3D objects work too; several of a kind:
    the strictest).  ValueError for CorrespondenceCheckerBasedOnNormal or
    anything else."""
    edge, dist = -1.0, -1.0
    for c in checkers or []:
        if hasattr(c, "normal_angle_threshold"):
            raise ValueError("CorrespondenceCheckerBasedOnNormal is not supported")
        if hasattr(c, "similarity_threshold"):
            edge = max(edge, float(c.similarity_threshold))
        elif hasattr(c, "distance_threshold"):
            d = float(c.distance_threshold)
            dist = d if dist < 0.0 else min(dist, d)
        else:
            raise ValueError(f"unsupported correspondence checker {c!r}")
    return edge, dist


class Feature:
    """Mirror of o3d.pipelines.registration.Feature: .data is the (dim, N)
    float64 array (Open3D's layout); the (N, dim) float32 device tensor the
    kernels produced stays in ._dev for the matcher."""

    def __init__(self, dev=None, data=None):
        self._dev = dev
        self._data = None if data is None else data

    @property
    def data(self):
        if self._data is None:
            import numpy as np

            self._data = np.ascontiguousarray(self._dev.detach().cpu().numpy().astype(np.float64).T)
        return self._data

    def device_rows(self):
        """(N, dim) float32 on the device."""
        if self._dev is None:
            import numpy as np
            import torch

            self._dev = torch.as_tensor(np.ascontiguousarray(np.asarray(self._data, np.float32).T),
                                        device=N.default_device())
        return self._dev

    def dimension(self) -> int:
        return int(self._dev.shape[1] if self._dev is not None else self._data.shape[0])

    def num(self) -> int:
        return int(self._dev.shape[0] if self._dev is not None else self._data.shape[1])

    def select_by_index(self, indices, invert: bool = False):
        """Open3D >= 0.18's Feature.select_by_index: a new Feature of the
        listed columns (invert: of every other column), in ascending column
        order.  On the device rows when they exist, else on .data (no GPU)."""
        import numpy as np

        if hasattr(indices, "detach"):
            indices = indices.detach().cpu().numpy()
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        n = self.num()
        if idx.size and (idx.min() < 0 or idx.max() >= n):
            raise IndexError(f"feature index outside [0, {n})")
        mask = np.zeros(n, dtype=bool)
        mask[idx] = True
        if invert:
            mask = ~mask
        sel = np.nonzero(mask)[0]
        if self._dev is not None:
            import torch

            rows = self._dev.index_select(0, torch.as_tensor(sel, device=self._dev.device)).contiguous()
            return Feature(dev=rows)
        return Feature(data=np.ascontiguousarray(np.asarray(self._data)[:, sel]))

    def __repr__(self):
        return f"Feature class with dimension = {self.dimension()} and num = {self.num()}"


def resolve(param):
    """-> (mode, knn, radius) for the C-ABI."""
    if param is None:
        return N.SEARCH_KNN, 30, 0.0
    has_r = hasattr(param, "radius")
    if has_r and hasattr(param, "max_nn"):
        return N.SEARCH_HYBRID, int(param.max_nn), float(param.radius)
    if has_r:
        return N.SEARCH_RADIUS, 0, float(param.radius)
    if hasattr(param, "knn"):
        return N.SEARCH_KNN, int(param.knn), 0.0
    raise TypeError(f"unsupported search parameter {param!r}")
