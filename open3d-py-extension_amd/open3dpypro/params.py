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
