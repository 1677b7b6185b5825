"""o3d.geometry.keypoint's module-level spelling: compute_iss_keypoints(pcd, ...)
-> a new cloud of the ISS keypoints (PointCloud.compute_iss_keypoints)."""
from __future__ import annotations


def compute_iss_keypoints(input, salient_radius: float = 0.0, non_max_radius: float = 0.0, gamma_21: float = 0.975,
                          gamma_32: float = 0.975, min_neighbors: int = 5):
    return input.compute_iss_keypoints(salient_radius=salient_radius, non_max_radius=non_max_radius,
                                       gamma_21=gamma_21, gamma_32=gamma_32, min_neighbors=min_neighbors)
