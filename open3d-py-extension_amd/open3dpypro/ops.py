"""Tensor-level hot-path ops: torch-ROCm tensors in, torch tensors out.

Each op is a thin call into libo3dx.so (include/o3dx.h); the tensor is only
the device array container.  Inputs: (N,3) contiguous on a ROCm GPU — float32,
or float64 for the float64 boundary (o3dx_*_f64: the hot-path ops computed on
the caller's float64 values, as Open3D computes them on its float64 storage).
PointCloud passes float64 only for clouds float32 cannot hold.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from . import _native as N


def _xyz(t: torch.Tensor, what="points") -> torch.Tensor:
    N.require_device(t, what)
    if t.ndim != 2 or t.shape[1] != 3:
        raise RuntimeError(f"{what} must have shape (n, 3), got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _is64(t) -> bool:
    return isinstance(t, torch.Tensor) and t.dtype == torch.float64


def _xyz64(t: torch.Tensor, what="points") -> torch.Tensor:
    N.require_device(t, what)
    if t.ndim != 2 or t.shape[1] != 3:
        raise RuntimeError(f"{what} must have shape (n, 3), got {tuple(t.shape)}")
    return t.to(torch.float64).contiguous()


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _np_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def aabb(xyz: torch.Tensor):
    """(min_bound, max_bound) as float64 numpy — get_min_bound/get_max_bound."""
    L = N.load()
    if _is64(xyz):
        x = _xyz64(xyz)
        n = x.shape[0]
        ws = N.workspace(L.o3dx_aabb_f64_workspace_bytes(n), x.device, "aabb")
        out = np.zeros(6, np.float64)
        N.check(L.o3dx_aabb_f64(N.ptr(x), n, _np_ptr(out), N.ptr(ws), ws.numel(), N.stream_ptr(x.device)), "aabb")
        return out[:3].copy(), out[3:].copy()
    x = _xyz(xyz)
    n = x.shape[0]
    ws = N.workspace(L.o3dx_aabb_workspace_bytes(n), x.device)
    out = np.zeros(6, np.float64)
    N.check(L.o3dx_aabb(N.ptr(x), n, _np_ptr(out), N.ptr(ws), ws.numel(), N.stream_ptr(x.device)), "aabb")
    return out[:3].copy(), out[3:].copy()


def aabb_device(xyz: torch.Tensor) -> torch.Tensor:
    """(6,) float64 device tensor {min, max} of the cloud, asynchronous
    (o3dx_aabb_device; zeros for an empty cloud)."""
    x = _xyz(xyz)
    L = N.load()
    n = x.shape[0]
    ws = N.workspace(L.o3dx_aabb_workspace_bytes(n), x.device, "aabb")
    out = torch.empty(6, dtype=torch.float64, device=x.device)
    N.check(L.o3dx_aabb_device(N.ptr(x), n, N.ptr(out), N.ptr(ws), ws.numel(), N.stream_ptr(x.device)), "aabb_device")
    return out


def voxel_down_sample(xyz: torch.Tensor, voxel_size: float, min_bound=None, max_bound=None,
                      with_xyz: bool = True, trace: bool = False, keep_grid: bool = False):
    """Open3D VoxelDownSampleAndTrace + idxmat.max(1) + _select_by_idx.

    Returns dict: rep_idx (M,) int32 ascending; rep_xyz (M,3) (if with_xyz);
    voxel_of_point (N,) int32 and cubic_id (M,8) int32 (if trace);
    voxel_grid (if keep_grid): the voxel table for estimate_normals(...,
    voxel_grid=) on the representatives' points (rep_xyz), or None when the
    grid was too sparse to keep.  float64 points: o3dx_voxel_down_sample_f64
    (keys from the float64 coordinates; rep_xyz float64; no voxel table)."""
    if _is64(xyz):
        return _voxel_down_sample_f64(xyz, voxel_size, min_bound, max_bound, with_xyz, trace, keep_grid)
    x = _xyz(xyz)
    L = N.load()
    n = x.shape[0]
    dev = x.device
    ws = N.workspace(L.o3dx_voxel_workspace_bytes(n), dev)
    rep = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    rxyz = torch.empty((max(n, 1), 3), dtype=torch.float32, device=dev) if with_xyz else None
    vop = torch.empty(max(n, 1), dtype=torch.int32, device=dev) if trace else None
    cub = torch.empty(max(8 * n, 8), dtype=torch.int32, device=dev) if trace else None
    mnb = None if min_bound is None else _c(min_bound, np.float64)
    mxb = None if max_bound is None else _c(max_bound, np.float64)
    m = np.zeros(1, np.int64)
    cells = 0
    if keep_grid and n > 0:
        # a table buffer for the largest grid the library keeps: the bounds
        # (and the AABB when they are not given) stay on the library's side,
        # no extra host round trip
        cells = int(L.o3dx_voxel_grid_capacity(n))
    geom = np.zeros(12, np.float64)
    if cells > 0:
        vox = torch.empty((cells, 4), dtype=torch.float32, device=dev)
        rc = L.o3dx_voxel_down_sample_grid(N.ptr(x), n, _np_ptr(mnb), _np_ptr(mxb), float(voxel_size), N.ptr(rep),
                                           N.ptr(rxyz), _np_ptr(m), N.ptr(vop), N.ptr(cub), N.ptr(vox), cells,
                                           _np_ptr(geom), N.ptr(ws), ws.numel(), N.stream_ptr(dev))
    else:
        rc = L.o3dx_voxel_down_sample(N.ptr(x), n, _np_ptr(mnb), _np_ptr(mxb), float(voxel_size), N.ptr(rep),
                                      N.ptr(rxyz), _np_ptr(m), N.ptr(vop), N.ptr(cub), N.ptr(ws), ws.numel(),
                                      N.stream_ptr(dev))
    N.check(rc, "voxel_down_sample")
    M = int(m[0])
    out = {"rep_idx": rep[:M]}
    if with_xyz:
        out["rep_xyz"] = rxyz[:M]
    if trace:
        out["voxel_of_point"] = vop[:n]
        out["cubic_id"] = cub[: 8 * M].view(M, 8)
    if keep_grid:
        out["voxel_grid"] = VoxelGrid(geom, vox, M) if geom[7] == 1.0 else None
    return out


def _voxel_down_sample_f64(xyz, voxel_size, min_bound, max_bound, with_xyz, trace, keep_grid):
    x = _xyz64(xyz)
    L = N.load()
    n = x.shape[0]
    dev = x.device
    ws = N.workspace(L.o3dx_voxel_f64_workspace_bytes(n), dev)
    rep = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    rxyz = torch.empty((max(n, 1), 3), dtype=torch.float64, device=dev) if with_xyz else None
    vop = torch.empty(max(n, 1), dtype=torch.int32, device=dev) if trace else None
    cub = torch.empty(max(8 * n, 8), dtype=torch.int32, device=dev) if trace else None
    mnb = None if min_bound is None else _c(min_bound, np.float64)
    mxb = None if max_bound is None else _c(max_bound, np.float64)
    m = np.zeros(1, np.int64)
    N.check(L.o3dx_voxel_down_sample_f64(N.ptr(x), n, _np_ptr(mnb), _np_ptr(mxb), float(voxel_size), N.ptr(rep),
                                         N.ptr(rxyz), _np_ptr(m), N.ptr(vop), N.ptr(cub), N.ptr(ws), ws.numel(),
                                         N.stream_ptr(dev)), "voxel_down_sample")
    M = int(m[0])
    out = {"rep_idx": rep[:M]}
    if with_xyz:
        out["rep_xyz"] = rxyz[:M]
    if trace:
        out["voxel_of_point"] = vop[:n]
        out["cubic_id"] = cub[: 8 * M].view(M, 8)
    if keep_grid:
        out["voxel_grid"] = None
    return out


def voxel_down_sample_window(xyz: torch.Tensor, voxel_size: float, min_bound, max_bound, kx0: int, kx1: int,
                             keep_grid: bool = False):
    """Slab form of voxel_down_sample (include/o3dx.h o3dx_voxel_down_sample_window):
    keys of the GLOBAL min_bound, only the x keys [kx0, kx1) materialised.
    Returns dict rep_idx, rep_xyz (and voxel_grid if keep_grid)."""
    x = _xyz(xyz)
    L = N.load()
    n = x.shape[0]
    dev = x.device
    ws = N.workspace(L.o3dx_voxel_workspace_bytes(n), dev)
    rep = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    rxyz = torch.empty((max(n, 1), 3), dtype=torch.float32, device=dev)
    m = np.zeros(1, np.int64)
    geom = np.zeros(12, np.float64)
    cells = int(L.o3dx_voxel_grid_capacity(n)) if keep_grid and n > 0 else 0
    vox = torch.empty((max(cells, 1), 4), dtype=torch.float32, device=dev) if cells else None
    N.check(L.o3dx_voxel_down_sample_window(N.ptr(x), n, _np_ptr(_c(min_bound, np.float64)),
                                            _np_ptr(_c(max_bound, np.float64)), float(voxel_size), int(kx0), int(kx1),
                                            N.ptr(rep), N.ptr(rxyz), _np_ptr(m), N.ptr(vox), cells, _np_ptr(geom),
                                            N.ptr(ws), ws.numel(), N.stream_ptr(dev)), "voxel_down_sample_window")
    M = int(m[0])
    out = {"rep_idx": rep[:M], "rep_xyz": rxyz[:M]}
    if keep_grid:
        out["voxel_grid"] = VoxelGrid(geom, vox, M) if geom[7] == 1.0 else None
    return out


def voxel_table(xyz: torch.Tensor, voxel_size: float, min_bound, max_bound, kx0: int, kx1: int,
                table: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None):
    """VoxelGrid of points holding at most one point per voxel (a slab's own +
    halo representatives), over the x-key window [kx0, kx1) of the global grid
    (o3dx_voxel_table_build).  `table`: an optional (cells, 4) float32 buffer.
    `status`: a zeroed int64 device tensor — the deferred form
    (o3dx_voxel_table_build_deferred): no host wait, non-finite rows skipped,
    error bits OR-ed into status[0] (1: a point outside the window, 2: two
    points in one voxel) for the caller to check."""
    x = _xyz(xyz)
    L = N.load()
    n = x.shape[0]
    dev = x.device
    mnb, mxb = _c(min_bound, np.float64), _c(max_bound, np.float64)
    dims = np.floor(np.maximum(mxb - mnb, 0.0) / voxel_size) + 1
    cells = int((kx1 - kx0) * dims[1] * dims[2])
    if table is None or table.shape[0] < cells:
        table = torch.empty((cells, 4), dtype=torch.float32, device=dev)
    geom = np.zeros(12, np.float64)
    ws = N.workspace(L.o3dx_voxel_table_workspace_bytes(), dev, "table")
    if status is not None:  # deferred: no host wait, error bits OR-ed into status[0] on the device
        N.check(L.o3dx_voxel_table_build_deferred(N.ptr(x), n, _np_ptr(mnb), _np_ptr(mxb), float(voxel_size),
                                                  int(kx0), int(kx1), N.ptr(table), table.shape[0], _np_ptr(geom),
                                                  N.ptr(status), N.stream_ptr(dev)), "voxel_table")
        return VoxelGrid(geom, table, n)
    N.check(L.o3dx_voxel_table_build(N.ptr(x), n, _np_ptr(mnb), _np_ptr(mxb), float(voxel_size), int(kx0), int(kx1),
                                     N.ptr(table), table.shape[0], _np_ptr(geom), N.ptr(ws), ws.numel(),
                                     N.stream_ptr(dev)), "voxel_table")
    return VoxelGrid(geom, table, n)


def voxel_down_sample_normals(xyz: torch.Tensor, voxel_size: float, knn: int = 30, min_bound=None, max_bound=None):
    """voxel_down_sample(keep_grid=True) + estimate_normals(KNN knn, voxel_grid=) on the
    representatives in one library call (o3dx_voxel_down_sample_normals): the
    normals are queued behind the voxel kernels without a host round trip.
    Returns dict rep_idx, rep_xyz, normals (M,3) float32, voxel_grid."""
    x = _xyz(xyz)
    L = N.load()
    n = x.shape[0]
    dev = x.device
    if n == 0:
        e = torch.empty((0, 3), dtype=torch.float32, device=dev)
        return {"rep_idx": torch.empty(0, dtype=torch.int32, device=dev), "rep_xyz": e, "normals": e.clone(),
                "voxel_grid": None}
    ws = N.workspace(L.o3dx_voxel_workspace_bytes(n), dev)
    nws = N.workspace(L.o3dx_normals_workspace_bytes(n), dev, "normals")
    rep = torch.empty(n, dtype=torch.int32, device=dev)
    rxyz = torch.empty((n, 3), dtype=torch.float32, device=dev)
    nrm = torch.empty((n, 3), dtype=torch.float32, device=dev)
    cells = int(L.o3dx_voxel_grid_capacity(n))
    vox = torch.empty((cells, 4), dtype=torch.float32, device=dev)
    mnb = None if min_bound is None else _c(min_bound, np.float64)
    mxb = None if max_bound is None else _c(max_bound, np.float64)
    m = np.zeros(1, np.int64)
    geom = np.zeros(12, np.float64)
    N.check(L.o3dx_voxel_down_sample_normals(N.ptr(x), n, _np_ptr(mnb), _np_ptr(mxb), float(voxel_size), int(knn),
                                             N.ptr(rep), N.ptr(rxyz), N.ptr(nrm), _np_ptr(m), N.ptr(vox), cells,
                                             _np_ptr(geom), N.ptr(ws), ws.numel(), N.ptr(nws), nws.numel(),
                                             N.stream_ptr(dev)), "voxel_down_sample_normals")
    M = int(m[0])
    return {"rep_idx": rep[:M], "rep_xyz": rxyz[:M], "normals": nrm[:M],
            "voxel_grid": VoxelGrid(geom, vox, M) if geom[7] == 1.0 else None}


class VoxelGrid:
    """The voxel table of a voxel_down_sample(keep_grid=True): per voxel the
    representative's (x, y, z, output row) (row -1 empty) + the grid geometry.
    Lets estimate_normals on the M representatives skip sorting them into a
    search grid (include/o3dx.h o3dx_estimate_normals_voxel)."""

    def __init__(self, geom: np.ndarray, pts: torch.Tensor, m: int):
        self.geom = np.ascontiguousarray(geom, np.float64)
        self.pts = pts
        self.m = int(m)


def estimate_normals(xyz: torch.Tensor, mode: int = N.SEARCH_KNN, knn: int = 30, radius: float = 0.0,
                     prior: Optional[torch.Tensor] = None, voxel_grid: Optional[VoxelGrid] = None,
                     return_kdist: bool = False):
    """Open3D EstimateNormals(search_param, fast_normal_computation=True) -> (N,3) float32.

    voxel_grid: the VoxelGrid of the voxel_down_sample that produced `xyz`
    (its rep_xyz); the search grid is then read off the voxel table.
    return_kdist (KNN only): also return (N,) float32 upper bounds of each
    point's squared k-th-neighbour distance (for halo checks of sharded runs).
    float64 points: o3dx_estimate_normals_f64 (sets and moments from the
    float64 coordinates; voxel_grid is not used)."""
    if _is64(xyz):
        return _estimate_normals_f64(xyz, mode, knn, radius, prior, return_kdist)
    x = _xyz(xyz)
    L = N.load()
    n = x.shape[0]
    dev = x.device
    out = torch.empty((max(n, 1), 3), dtype=torch.float32, device=dev)
    if return_kdist and mode != N.SEARCH_KNN:
        raise ValueError("return_kdist needs KNN search")
    kd2 = torch.empty(max(n, 1), dtype=torch.float32, device=dev) if return_kdist else None
    pr = None if prior is None else _xyz(prior.to(dev), "prior normals")
    ws = N.workspace(L.o3dx_normals_workspace_bytes(n), dev)
    if voxel_grid is not None:
        if voxel_grid.m != n or voxel_grid.pts.device != dev:
            raise ValueError("voxel_grid does not belong to these points")
        rc = L.o3dx_estimate_normals_voxel(_np_ptr(voxel_grid.geom), N.ptr(voxel_grid.pts), N.ptr(x), n, int(mode),
                                           int(knn), float(radius), N.ptr(pr), N.ptr(out), N.ptr(kd2), N.ptr(ws),
                                           ws.numel(), N.stream_ptr(dev))
    else:
        rc = L.o3dx_estimate_normals(N.ptr(x), n, int(mode), int(knn), float(radius), N.ptr(pr), N.ptr(out),
                                     N.ptr(kd2), N.ptr(ws), ws.numel(), N.stream_ptr(dev))
    N.check(rc, "estimate_normals")
    if return_kdist:
        return out[:n], kd2[:n]
    return out[:n]


def _estimate_normals_f64(xyz, mode, knn, radius, prior, return_kdist):
    x = _xyz64(xyz)
    L = N.load()
    n = x.shape[0]
    dev = x.device
    if return_kdist and mode != N.SEARCH_KNN:
        raise ValueError("return_kdist needs KNN search")
    out = torch.empty((max(n, 1), 3), dtype=torch.float32, device=dev)
    kd2 = torch.empty(max(n, 1), dtype=torch.float32, device=dev) if return_kdist else None
    pr = None if prior is None else _xyz(prior.to(dev), "prior normals")
    ws = N.workspace(L.o3dx_normals_f64_workspace_bytes(n), dev)
    N.check(L.o3dx_estimate_normals_f64(N.ptr(x), n, int(mode), int(knn), float(radius), N.ptr(pr), N.ptr(out),
                                        N.ptr(kd2), N.ptr(ws), ws.numel(), N.stream_ptr(dev)), "estimate_normals")
    if return_kdist:
        return out[:n], kd2[:n]
    return out[:n]


def knn_search(xyz: torch.Tensor, queries: torch.Tensor, mode: int = N.SEARCH_KNN, knn: int = 30,
               radius: float = 0.0):
    """Batched KDTreeFlann search: (idx (nq,K) int32, d2 (nq,K) float64, count (nq,) int32).
    float64 points: o3dx_knn_search_f64 (queries taken as float64)."""
    if _is64(xyz):
        x = _xyz64(xyz)
        q = _xyz64(queries.to(x.device), "queries")
        L = N.load()
        n, nq = x.shape[0], q.shape[0]
        dev = x.device
        K = int(knn)
        idx = torch.empty((max(nq, 1), K), dtype=torch.int32, device=dev)
        d2 = torch.empty((max(nq, 1), K), dtype=torch.float64, device=dev)
        cnt = torch.empty(max(nq, 1), dtype=torch.int32, device=dev)
        ws = N.workspace(L.o3dx_knn_f64_workspace_bytes(n), dev)
        N.check(L.o3dx_knn_search_f64(N.ptr(x), n, N.ptr(q), nq, int(mode), K, float(radius), N.ptr(idx), N.ptr(d2),
                                      N.ptr(cnt), N.ptr(ws), ws.numel(), N.stream_ptr(dev)), "knn_search")
        return idx[:nq], d2[:nq], cnt[:nq]
    x = _xyz(xyz)
    q = _xyz(queries.to(x.device), "queries")
    L = N.load()
    n, nq = x.shape[0], q.shape[0]
    dev = x.device
    K = int(knn)
    idx = torch.empty((max(nq, 1), K), dtype=torch.int32, device=dev)
    d2 = torch.empty((max(nq, 1), K), dtype=torch.float64, device=dev)
    cnt = torch.empty(max(nq, 1), dtype=torch.int32, device=dev)
    ws = N.workspace(L.o3dx_knn_workspace_bytes(n), dev)
    rc = L.o3dx_knn_search(N.ptr(x), n, N.ptr(q), nq, int(mode), K, float(radius), N.ptr(idx), N.ptr(d2), N.ptr(cnt),
                           N.ptr(ws), ws.numel(), N.stream_ptr(dev))
    N.check(rc, "knn_search")
    return idx[:nq], d2[:nq], cnt[:nq]


def search_one(xyz: torch.Tensor, query, mode: int = N.SEARCH_KNN, knn: int = 30, radius: float = 0.0):
    """One KDTreeFlann query of any size (o3dx_search_one): (k, idx (k,) int32,
    d2 (k,) float64) on the device, sorted by (d^2, index).  mode KNN: the knn
    nearest; RADIUS: every point with d^2 < radius^2; HYBRID: the knn nearest
    of those.  float32 or float64 points (the cloud's own coordinates)."""
    f64 = _is64(xyz)
    x = _xyz64(xyz) if f64 else _xyz(xyz)
    L = N.load()
    n = x.shape[0]
    q = _c(np.asarray(query, np.float64).reshape(3), np.float64)
    cap = n if mode == N.SEARCH_RADIUS else min(int(knn), n)
    idx = torch.empty(max(cap, 1), dtype=torch.int32, device=x.device)
    d2 = torch.empty(max(cap, 1), dtype=torch.float64, device=x.device)
    cnt = np.zeros(1, np.int64)
    ws = N.workspace(L.o3dx_search_one_workspace_bytes(n), x.device, "search")
    N.check(L.o3dx_search_one(N.ptr(x), 1 if f64 else 0, n, _np_ptr(q), int(mode), int(knn), float(radius),
                              N.ptr(idx), N.ptr(d2), cap, _np_ptr(cnt), N.ptr(ws), ws.numel(),
                              N.stream_ptr(x.device)), "search_one")
    k = int(cnt[0])
    return k, idx[:k], d2[:k]


def dbscan(xyz: torch.Tensor, eps: float, min_samples: int, return_core: bool = False):
    """sklearn.cluster.DBSCAN(eps, min_samples).fit(xyz) on the device
    (o3dx_dbscan; include/o3dx.h states the rule): (labels (n,) int32 device
    tensor, n_clusters[, core (n,) bool device tensor]).  Labels are sklearn's:
    clusters numbered by ascending smallest core index, noise -1.  float64
    points: o3dx_dbscan_f64 (every pair decided on the float64 coordinates).
    ValueError, as sklearn, for eps <= 0, min_samples < 1 or no points."""
    eps = float(eps)
    if not (eps > 0.0) or not np.isfinite(eps):
        raise ValueError(f"eps must be a finite float > 0, got {eps}")
    if int(min_samples) != min_samples or int(min_samples) < 1:
        raise ValueError(f"min_samples must be an int >= 1, got {min_samples}")
    if isinstance(xyz, torch.Tensor) and xyz.ndim == 2 and xyz.shape[0] == 0:
        raise ValueError("dbscan: found a cloud with 0 points (a minimum of 1 is required)")
    f64 = _is64(xyz)
    x = _xyz64(xyz) if f64 else _xyz(xyz)
    L = N.load()
    n = x.shape[0]
    dev = x.device
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    core = torch.empty(n, dtype=torch.uint8, device=dev) if return_core else None
    cnt = np.zeros(1, np.int64)
    if f64:
        ws = N.workspace(L.o3dx_dbscan_f64_workspace_bytes(n), dev)
        fn = L.o3dx_dbscan_f64
    else:
        ws = N.workspace(L.o3dx_dbscan_workspace_bytes(n), dev)
        fn = L.o3dx_dbscan
    N.check(fn(N.ptr(x), n, eps, int(min_samples), N.ptr(labels), N.ptr(core), _np_ptr(cnt), N.ptr(ws), ws.numel(),
               N.stream_ptr(dev)), "dbscan")
    if return_core:
        return labels, int(cnt[0]), core.bool()
    return labels, int(cnt[0])


def emst(xyz: torch.Tensor) -> torch.Tensor:
    """The Euclidean minimum spanning tree of the points (o3dx_emst): an
    (n - 1, 2) int32 device tensor of {lo, hi} rows, lo < hi, sorted by
    (lo, hi).  Weights are the float64 d^2 of the float32 coordinates; edges
    are compared by (d^2, lo, hi), so the tree is unique even with duplicate
    points.  float32 points only."""
    if _is64(xyz):
        raise NotImplementedError("emst: float64 clouds are outside this implementation (float32 points only)")
    x = _xyz(xyz)
    n = x.shape[0]
    dev = x.device
    edges = torch.empty((max(n - 1, 0), 2), dtype=torch.int32, device=dev)
    if n < 2:
        return edges
    L = N.load()
    ws = N.workspace(L.o3dx_emst_workspace_bytes(n), dev)
    N.check(L.o3dx_emst(N.ptr(x), n, None, 0, N.ptr(edges), N.ptr(ws), ws.numel(), N.stream_ptr(dev)), "emst")
    return edges


def orient_normals_tangent_plane(xyz: torch.Tensor, normals: torch.Tensor, k: int, return_tree: bool = False):
    """Open3D OrientNormalsConsistentTangentPlane(k) on the device
    (o3dx_orient_normals_tangent_plane; include/o3dx.h states the rule):
    the oriented normals, a new (n, 3) float32 tensor whose rows are the
    input's or their negation (sign bits only).  return_tree: also the
    (n - 1, 2) int32 tree edges sorted by (lo, hi) and the (n,) bool flips.
    The neighbour lists are knn_search's (min(k, n) nearest, the point itself
    included; at most MAX_KNN).  ValueError for k < 1; float32 points only."""
    if int(k) != k or int(k) < 1:
        raise ValueError(f"k must be an int >= 1, got {k}")
    if _is64(xyz):
        raise NotImplementedError("orient_normals_tangent_plane: float64 clouds are outside this implementation "
                                  "(float32 points only)")
    x = _xyz(xyz)
    nrm = _xyz(normals, "normals")
    n = x.shape[0]
    if nrm.shape[0] != n:
        raise RuntimeError(f"normals must have one row per point ({n}), got {nrm.shape[0]}")
    dev = x.device
    out = nrm.clone()
    tree = torch.empty((max(n - 1, 0), 2), dtype=torch.int32, device=dev)
    flipped = torch.zeros(n, dtype=torch.uint8, device=dev)
    if n > 0:
        kk = min(int(k), n)
        idx, _, _ = knn_search(x, x, N.SEARCH_KNN, kk)
        idx = idx.contiguous()
        L = N.load()
        ws = N.workspace(L.o3dx_orient_normals_workspace_bytes(n, kk), dev)
        N.check(L.o3dx_orient_normals_tangent_plane(N.ptr(x), n, N.ptr(idx), kk, N.ptr(out),
                                                    N.ptr(tree) if return_tree and n > 1 else None,
                                                    N.ptr(flipped) if return_tree else None, N.ptr(ws), ws.numel(),
                                                    N.stream_ptr(dev)), "orient_normals_tangent_plane")
    if return_tree:
        return out, tree, flipped.bool()
    return out


def raster2d_size(resolution: float, minx: float, miny: float, maxx: float, maxy: float):
    """(w, h) of the reference's to_2D_Img image for these x / y bounds
    (o3dx_raster2d_size, host only; either may be 0)."""
    wh = np.zeros(2, np.int64)
    b = _c([minx, miny, maxx, maxy], np.float64)
    N.check(N.load().o3dx_raster2d_size(float(resolution), _np_ptr(b), _np_ptr(wh)), "raster2d_size")
    return int(wh[0]), int(wh[1])


def raster2d(xyz: torch.Tensor, resolution: float, want_winner: bool = False):
    """The reference's to_2D_Img rasterisation (PointCloud.py:785-823) on the
    device (o3dx_raster2d / o3dx_raster2d_f64 by the points' dtype;
    include/o3dx.h states the rule).  Returns a dict of device tensors and
    host scalars: pix (n,2) int32 {ix, iy}, img (h,w) uint8 (255 on a hit
    pixel), winner (h,w) int32 (the highest point index per pixel, -1 when
    empty; None unless want_winner), minx, miny (float64), w, h.
    ValueError for a resolution <= 0 or not finite and for an empty cloud;
    IndexError when the image would have no column or no row (all points in
    one pixel column or row), as the reference's indexing raises."""
    resolution = float(resolution)
    if not (resolution > 0.0) or not np.isfinite(resolution):
        raise ValueError(f"resolution must be a finite float > 0, got {resolution}")
    if isinstance(xyz, torch.Tensor) and xyz.ndim == 2 and xyz.shape[0] == 0:
        raise ValueError("raster2d: found a cloud with 0 points (a minimum of 1 is required)")
    f64 = _is64(xyz)
    x = _xyz64(xyz) if f64 else _xyz(xyz)
    mn, mx = aabb(x)
    if not (np.isfinite(mn).all() and np.isfinite(mx).all()):
        raise ValueError("raster2d: the coordinates must be finite")
    L = N.load()
    n = x.shape[0]
    dev = x.device
    w, h = raster2d_size(resolution, mn[0], mn[1], mx[0], mx[1])
    if w < 1 or h < 1:
        raise IndexError(f"raster2d: the image would be {h} x {w} (all points in one pixel row or column)")
    b = _c([mn[0], mn[1], mx[0], mx[1]], np.float64)
    pix = torch.empty((n, 2), dtype=torch.int32, device=dev)
    img = torch.empty((h, w), dtype=torch.uint8, device=dev)
    winner = torch.empty((h, w), dtype=torch.int32, device=dev) if want_winner else None
    fn = L.o3dx_raster2d_f64 if f64 else L.o3dx_raster2d
    N.check(fn(N.ptr(x), n, resolution, _np_ptr(b), N.ptr(pix), N.ptr(img), N.ptr(winner), w * h,
               N.stream_ptr(dev)), "raster2d")
    return {"pix": pix, "img": img, "winner": winner, "minx": np.float64(mn[0]), "miny": np.float64(mn[1]),
            "w": w, "h": h}


def ccl2d(img: torch.Tensor):
    """8-connected components of a 2-D uint8 device image (o3dx_ccl2d): a
    non-zero pixel is foreground, label 0 the background, components numbered
    1, 2, ... by ascending row-major position of their first pixel.  Returns
    (labels (h,w) int32, areas (k+1,) int64 — areas[0] the zero pixels —, k),
    the first two on the device."""
    N.require_device(img, "img")
    if img.ndim != 2 or img.dtype != torch.uint8:
        raise RuntimeError(f"img must be a 2-D uint8 tensor, got {tuple(img.shape)} {img.dtype}")
    im = img.contiguous()
    L = N.load()
    h, w = int(im.shape[0]), int(im.shape[1])
    dev = im.device
    labels = torch.empty((h, w), dtype=torch.int32, device=dev)
    areas = torch.empty(int(L.o3dx_ccl2d_max_labels(w, h)) + 1, dtype=torch.int64, device=dev)
    k = np.zeros(1, np.int64)
    ws = N.workspace(int(L.o3dx_ccl2d_workspace_bytes(w, h)), dev)
    N.check(L.o3dx_ccl2d(N.ptr(im), w, h, N.ptr(labels), N.ptr(areas), _np_ptr(k), N.ptr(ws), ws.numel(),
                         N.stream_ptr(dev)), "ccl2d")
    return labels, areas[: int(k[0]) + 1], int(k[0])


def label_group(pix: torch.Tensor, labels: torch.Tensor, k: int):
    """The points grouped by the label of their pixel (o3dx_label_group): pix
    (n,2) int32 {ix, iy}, labels (h,w) int32 with values in [0, k].  Returns
    device tensors (point_label (n,) int32, order (n,) int32 — the point
    indices grouped by label, ascending inside each —, counts (k+1,) int64).
    RuntimeError (EINVAL) when a pixel lies outside the image."""
    N.require_device(pix, "pix")
    N.require_device(labels, "labels")
    if pix.ndim != 2 or pix.shape[1] != 2 or labels.ndim != 2:
        raise RuntimeError(f"pix must be (n,2) and labels (h,w), got {tuple(pix.shape)} and {tuple(labels.shape)}")
    px = pix.to(torch.int32).contiguous()
    lb = labels.to(torch.int32).contiguous()
    L = N.load()
    n = int(px.shape[0])
    h, w = int(lb.shape[0]), int(lb.shape[1])
    dev = px.device
    point_label = torch.empty(n, dtype=torch.int32, device=dev)
    order = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty(int(k) + 1, dtype=torch.int64, device=dev)
    ws = N.workspace(int(L.o3dx_label_group_workspace_bytes(n, int(k))), dev)
    N.check(L.o3dx_label_group(N.ptr(px), n, N.ptr(lb), w, h, int(k), N.ptr(point_label), N.ptr(order),
                               N.ptr(counts), N.ptr(ws), ws.numel(), N.stream_ptr(dev)), "label_group")
    return point_label, order, counts


def las_unpack(records: torch.Tensor, n: int, stride: int, point_format: int, scales, offsets, rgb: bool = False,
               intensity: bool = False, labels: bool = False):
    """LAS point records decoded on the device (o3dx_las_unpack;
    include/o3dx.h states the layout and the rules).  records: a uint8 device
    tensor of at least n * stride bytes.  Returns a dict of device tensors:
    points64 (n,3) float64 = X * scale + offset, points32 (n,3) float32, flags
    (1,) int32 (bit 0: some coordinate is not a float32 value), and when asked
    for rgb (n,3) float32 = u16 / 65536, intensity (n,) int16 holding the raw
    u16 bits, labels (n,) uint8 (the whole classification byte).  No host
    wait: reading flags is the caller's."""
    N.require_device(records, "records")
    n, stride = int(n), int(stride)
    if records.dtype != torch.uint8 or n < 0 or records.numel() < n * stride:
        raise RuntimeError(f"records must be a uint8 tensor of >= n * stride = {n * stride} bytes, got "
                           f"{records.dtype} x {records.numel()}")
    rec = records.contiguous()
    dev = rec.device
    p64 = torch.empty((n, 3), dtype=torch.float64, device=dev)
    p32 = torch.empty((n, 3), dtype=torch.float32, device=dev)
    flags = torch.empty(1, dtype=torch.int32, device=dev)
    col = torch.empty((n, 3), dtype=torch.float32, device=dev) if rgb else None
    inten = torch.empty(n, dtype=torch.int16, device=dev) if intensity else None
    cls = torch.empty(n, dtype=torch.uint8, device=dev) if labels else None
    sc, of = _c(scales, np.float64).reshape(3), _c(offsets, np.float64).reshape(3)
    N.check(N.load().o3dx_las_unpack(N.ptr(rec), n, stride, int(point_format), _np_ptr(sc), _np_ptr(of), N.ptr(p64),
                                     N.ptr(p32), N.ptr(inten), N.ptr(cls), N.ptr(col), N.ptr(flags),
                                     N.stream_ptr(dev)), "las_unpack")
    return {"points64": p64, "points32": p32, "flags": flags, "rgb": col, "intensity": inten, "labels": cls}


def las_pack(xyz: torch.Tensor, stride: int, point_format: int, scales, offsets, rgb: Optional[torch.Tensor] = None,
             intensity: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None):
    """LAS point records encoded on the device (o3dx_las_pack): xyz (n,3)
    float32 or float64, rgb (n,3) float32 in [0,1], intensity (n,) int16 /
    uint16 bits, labels (n,) uint8.  Returns (records (n, stride) uint8,
    stats (8,) int64 {min X Y Z, max X Y Z, values outside int32, non-finite
    values}), both on the device and not waited for."""
    f64 = _is64(xyz)
    x = _xyz64(xyz) if f64 else _xyz(xyz)
    n, stride = int(x.shape[0]), int(stride)
    dev = x.device

    def opt(t, dtypes, shape, what):
        if t is None:
            return None
        N.require_device(t, what)
        if t.dtype not in dtypes or tuple(t.shape) != shape:
            raise RuntimeError(f"{what} must be {dtypes[0]} of shape {shape}, got {t.dtype} {tuple(t.shape)}")
        return t.contiguous()

    col = opt(rgb, (torch.float32,), (n, 3), "rgb")
    inten = opt(intensity, (torch.int16, getattr(torch, "uint16", torch.int16)), (n,), "intensity")
    cls = opt(labels, (torch.uint8,), (n,), "labels")
    rec = torch.empty((n, max(stride, 0)), dtype=torch.uint8, device=dev)
    stats = torch.empty(8, dtype=torch.int64, device=dev)
    sc, of = _c(scales, np.float64).reshape(3), _c(offsets, np.float64).reshape(3)
    N.check(N.load().o3dx_las_pack(N.ptr(x), 1 if f64 else 0, n, stride, int(point_format), _np_ptr(sc), _np_ptr(of),
                                   N.ptr(col), N.ptr(inten), N.ptr(cls), N.ptr(rec), N.ptr(stats),
                                   N.stream_ptr(dev)), "las_pack")
    return rec, stats


def _e57_bytes(t: torch.Tensor, what: str) -> torch.Tensor:
    N.require_device(t, what)
    if t.dtype != torch.uint8 or t.ndim != 1:
        raise RuntimeError(f"{what} must be a 1-d uint8 tensor, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def e57_crc_pages(file_bytes: torch.Tensor):
    """CRC32C of every whole 1024-byte page of an E57 file's bytes against its
    big-endian trailer, on the device (o3dx_e57_crc_pages).  Returns (bad
    pages, first bad page or -1) as Python ints (waits)."""
    f = _e57_bytes(file_bytes, "file_bytes")
    out = torch.empty(2, dtype=torch.int64, device=f.device)
    N.check(N.load().o3dx_e57_crc_pages(N.ptr(f), f.numel() // 1024, N.ptr(out), N.stream_ptr(f.device)),
            "e57_crc_pages")
    bad, first = out.cpu().tolist()
    return int(bad), int(first) if bad else -1


def e57_unpack(file_bytes: torch.Tensor, desc, affine, segments, r0: int, n: int, pose=None):
    """Records [r0, r0 + n) of one E57 scan decoded on the device from the
    paged file bytes (o3dx_e57_unpack; include/o3dx.h states the rules).
    desc (k,6) int64 {role, kind, bits, minimum, first segment row, segment
    rows}, affine (k,2) float64 {scale, offset}, segments (m,3) int64 {stream
    byte offset, logical file offset, length} (e57_io.field_tables); pose: 12
    float64 (R row-major, t) or None.  Returns device tensors for the roles
    present: points64 / points32 (n,3), rgb (n,3) uint8, intensity (n,)
    float32, row / col (n,) int16 holding the u16 bits, invalid (n,) int8
    (None otherwise), and flags (1,) int32 (bit 0: some coordinate is not a
    float32 value; bit 1: a record's bytes lie outside its segments or the
    file).  No host wait: reading flags is the caller's."""
    f = _e57_bytes(file_bytes, "file_bytes")
    dev = f.device
    d = _c(desc, np.int64).reshape(-1, 6)
    a = _c(affine, np.float64).reshape(-1, 2)
    sg = _c(segments, np.int64).reshape(-1, 3)
    if len(a) != len(d):
        raise RuntimeError(f"affine must have one row per field ({len(d)}), got {len(a)}")
    r0, n = int(r0), int(n)
    if n < 0:
        raise RuntimeError(f"n must be >= 0, got {n}")
    seg = torch.from_numpy(sg).to(dev) if len(sg) else None
    roles = set(int(r) for r in d[:, 0])
    xyz = {0, 1, 2} <= roles
    new = lambda ok, shape, dt: torch.empty(shape, dtype=dt, device=dev) if ok else None  # noqa: E731
    p64, p32 = new(xyz, (n, 3), torch.float64), new(xyz, (n, 3), torch.float32)
    col = new({4, 5, 6} <= roles, (n, 3), torch.uint8)
    inten = new(3 in roles, (n,), torch.float32)
    row, cl = new(7 in roles, (n,), torch.int16), new(8 in roles, (n,), torch.int16)
    inv = new(9 in roles, (n,), torch.int8)
    flags = torch.empty(1, dtype=torch.int32, device=dev)
    ps = None if pose is None else _c(pose, np.float64).reshape(12)
    N.check(N.load().o3dx_e57_unpack(N.ptr(f), f.numel(), len(d), _np_ptr(d), _np_ptr(a), N.ptr(seg), len(sg), r0, n,
                                     _np_ptr(ps), N.ptr(p64), N.ptr(p32), N.ptr(col), N.ptr(inten), N.ptr(row),
                                     N.ptr(cl), N.ptr(inv), N.ptr(flags), N.stream_ptr(dev)), "e57_unpack")
    return {"points64": p64, "points32": p32, "rgb": col, "intensity": inten, "row": row, "col": cl, "invalid": inv,
            "flags": flags}


def e57_pack(desc, sources, n: int, records_per_packet: int, full_bytes: int, last_bytes: int, head_full: bytes,
             head_last: bytes, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One E57 scan's data packets, headers included, encoded on the device
    (o3dx_e57_pack).  desc (k,6) int64 {source kind, bits, minimum, stream
    offset in a full packet, in the last packet, stream bytes in the last
    packet} and the packet geometry come from e57_io.ScanPlan; sources: per
    field (tensor, element stride, first element) — float32, float64 or int64
    device tensors as the source kind says.  Returns the packets as a uint8
    tensor ((packets - 1) * full_bytes + last_bytes bytes; `out`, a 4-byte
    aligned uint8 tensor of that size, is filled when given).  Not waited for."""
    d = _c(desc, np.int64).reshape(-1, 6)
    n, R = int(n), int(records_per_packet)
    if len(sources) != len(d) or not len(d):
        raise RuntimeError(f"sources must have one entry per field ({len(d)}), got {len(sources)}")
    want = {0: torch.float32, 1: torch.float64, 2: torch.float32, 3: torch.int64}
    keep, ptrs, strides = [], [], np.zeros((len(d), 2), np.int64)
    dev = None
    for k, (t, stride, first) in enumerate(sources):
        N.require_device(t, f"source {k}")
        if t.dtype != want.get(int(d[k, 0])):
            raise RuntimeError(f"source {k} must be {want.get(int(d[k, 0]))} for source kind {int(d[k, 0])}, got "
                               f"{t.dtype}")
        t = t.contiguous()
        if n and (int(first) < 0 or int(stride) < 0 or int(first) + (n - 1) * int(stride) >= t.numel()):
            raise RuntimeError(f"source {k}: {n} records at stride {stride} from element {first} leave its "
                               f"{t.numel()} elements")
        keep.append(t)
        ptrs.append(t.data_ptr())
        strides[k] = (int(stride), int(first))
        dev = t.device
    packets = (n + R - 1) // R if R > 0 else 0
    size = (packets - 1) * int(full_bytes) + int(last_bytes) if packets else 0
    if out is None:
        out = torch.empty(size, dtype=torch.uint8, device=dev)
    else:
        N.require_device(out, "out")
        if out.dtype != torch.uint8 or out.numel() != size or not out.is_contiguous():
            raise RuntimeError(f"out must be a contiguous uint8 tensor of {size} bytes")
    arr = (ctypes.c_void_p * len(d))(*ptrs)
    hf, hl = _c(np.frombuffer(bytes(head_full), np.uint8), np.uint8), _c(np.frombuffer(bytes(head_last), np.uint8),
                                                                         np.uint8)
    if len(hf) != 6 + 2 * len(d) or len(hl) != len(hf):
        raise RuntimeError(f"packet headers must be {6 + 2 * len(d)} bytes, got {len(hf)} and {len(hl)}")
    N.check(N.load().o3dx_e57_pack(len(d), _np_ptr(d), ctypes.cast(arr, ctypes.c_void_p), _np_ptr(strides), n, R,
                                   int(full_bytes), int(last_bytes), _np_ptr(hf), _np_ptr(hl), N.ptr(out),
                                   N.stream_ptr(dev)), "e57_pack")
    del keep
    return out


def e57_seal(logical_bytes: torch.Tensor) -> torch.Tensor:
    """Logical bytes laid into 1024-byte E57 pages, each with its CRC32C
    trailer, on the device (o3dx_e57_seal); the last page is zero-padded."""
    lg = _e57_bytes(logical_bytes, "logical_bytes")
    if lg.numel() % 4:
        lg = torch.cat([lg, torch.zeros(4 - lg.numel() % 4, dtype=torch.uint8, device=lg.device)])
    pages = (lg.numel() + 1019) // 1020
    out = torch.empty(pages * 1024, dtype=torch.uint8, device=lg.device)
    N.check(N.load().o3dx_e57_seal(N.ptr(lg), lg.numel(), N.ptr(out), pages, N.stream_ptr(lg.device)), "e57_seal")
    return out


def ransac_samples(n: int, ransac_n: int, num_iterations: int, seed: int) -> np.ndarray:
    """Open3D RandomSampler over mt19937(seed): (iters, ransac_n) int32."""
    out = np.empty((max(num_iterations, 1), ransac_n), np.int32)
    N.check(N.load().o3dx_ransac_samples(int(n), int(ransac_n), int(num_iterations), int(seed) & (2**64 - 1),
                                         _np_ptr(out)), "ransac_samples")
    return out[:num_iterations]


def segment_plane(xyz: torch.Tensor, distance_threshold: float, ransac_n: int, num_iterations: int,
                  probability: float = 0.99999999, samples: Optional[np.ndarray] = None, seed: int = 0):
    """Open3D SegmentPlane -> (plane float64[4], inliers (k,) int32 ascending on device).
    float64 points: o3dx_segment_plane_f64 (exact counts on the float64 coordinates)."""
    f64 = _is64(xyz)
    x = _xyz64(xyz) if f64 else _xyz(xyz)
    L = N.load()
    n = x.shape[0]
    dev = x.device
    if not (0.0 < probability <= 1.0):
        raise RuntimeError("Probability must be > 0 or <= 1.0")
    if ransac_n < 3:
        raise RuntimeError("ransac_n should be set to higher than or equal to 3.")
    if n < ransac_n:
        raise RuntimeError("There must be at least 'ransac_n' points.")
    if samples is None:
        samples = ransac_samples(n, ransac_n, num_iterations, seed)
    s = _c(samples, np.int32).reshape(num_iterations, ransac_n)
    plane = np.zeros(4, np.float64)
    inl = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    k = np.zeros(1, np.int64)
    wsb = (L.o3dx_segment_plane_f64_workspace_bytes if f64 else L.o3dx_segment_plane_workspace_bytes)
    ws = N.workspace(wsb(n, num_iterations), dev)
    fn = L.o3dx_segment_plane_f64 if f64 else L.o3dx_segment_plane
    rc = fn(N.ptr(x), n, float(distance_threshold), int(ransac_n), int(num_iterations), float(probability),
            _np_ptr(s), _np_ptr(plane), N.ptr(inl), _np_ptr(k), N.ptr(ws), ws.numel(), N.stream_ptr(dev))
    N.check(rc, "segment_plane")
    return plane, inl[: int(k[0])]


def plane_count(xyz: torch.Tensor, planes: np.ndarray, distance_threshold: float) -> np.ndarray:
    """Exact per-hypothesis inlier counts (-1 for degenerate planes); float64
    points: o3dx_plane_count_f64."""
    f64 = _is64(xyz)
    x = _xyz64(xyz) if f64 else _xyz(xyz)
    L = N.load()
    n = x.shape[0]
    P = _c(planes, np.float64).reshape(-1, 4)
    H = P.shape[0]
    counts = np.zeros(max(H, 1), np.int64)
    ws = N.workspace(L.o3dx_plane_count_workspace_bytes(n, H), x.device)
    fn = L.o3dx_plane_count_f64 if f64 else L.o3dx_plane_count
    N.check(fn(N.ptr(x), n, _np_ptr(P), H, float(distance_threshold), _np_ptr(counts), N.ptr(ws),
                               ws.numel(), N.stream_ptr(x.device)), "plane_count")
    return counts[:H]


def plane_count_upper(xyz: torch.Tensor, planes: np.ndarray, distance_threshold: float, absmax=None) -> np.ndarray:
    """Upper bounds of the per-hypothesis inlier counts (>= exact; -1 for
    degenerate planes), o3dx_plane_count_upper; absmax: the cloud's |x|,|y|,|z|
    bounds (None: its own)."""
    x = _xyz(xyz)
    L = N.load()
    n = x.shape[0]
    P = _c(planes, np.float64).reshape(-1, 4)
    H = P.shape[0]
    counts = np.zeros(max(H, 1), np.int64)
    am = None if absmax is None else _c(absmax, np.float64)
    ws = N.workspace(L.o3dx_plane_count_workspace_bytes(n, H), x.device)
    N.check(L.o3dx_plane_count_upper(N.ptr(x), n, _np_ptr(P), H, float(distance_threshold),
                                     None if am is None else _np_ptr(am), _np_ptr(counts), N.ptr(ws), ws.numel(),
                                     N.stream_ptr(x.device)), "plane_count_upper")
    return counts[:H]


def ransac_needed(counts, known, planes, n: int, ransac_n: int, probability: float = 0.99999999) -> np.ndarray:
    """The hypotheses without an exact count (known False) that Open3D's
    selection replay on `counts` consults (o3dx_ransac_needed); empty: the
    selection on these counts is the exact one."""
    c = _c(counts, np.int64)
    k8 = _c(np.asarray(known, bool).astype(np.uint8), np.uint8)
    P = _c(planes, np.float64).reshape(-1, 4)
    out = np.zeros(max(len(c), 1), np.int32)
    k = np.zeros(1, np.int32)
    N.check(N.load().o3dx_ransac_needed(_np_ptr(c), _np_ptr(k8), _np_ptr(P), len(c), int(n), int(ransac_n),
                                        float(probability), _np_ptr(out), _np_ptr(k)), "ransac_needed")
    return out[: int(k[0])].copy()


def plane_abs_sum(xyz: torch.Tensor, planes: np.ndarray, which, distance_threshold: float, return_fx: bool = False):
    """Sigma |d| over |d| < thr of the hypotheses `which` (exact fx sums):
    float64 (L,), and with return_fx their (L, 4) int64 fx rows."""
    x = _xyz(xyz)
    L = N.load()
    n = x.shape[0]
    P = _c(planes, np.float64).reshape(-1, 4)
    w = _c(which, np.int32)
    sums = np.zeros(max(len(w), 1), np.float64)
    fx = np.zeros((max(len(w), 1), 4), np.int64)
    ws = N.workspace(L.o3dx_plane_count_workspace_bytes(n, max(len(w), 1)), x.device)
    N.check(L.o3dx_plane_abs_sum(N.ptr(x), n, _np_ptr(P), _np_ptr(w), len(w), float(distance_threshold),
                                 _np_ptr(sums), _np_ptr(fx), N.ptr(ws), ws.numel(), N.stream_ptr(x.device)),
            "plane_abs_sum")
    return (sums[: len(w)], fx[: len(w)]) if return_fx else sums[: len(w)]


def ransac_tied(counts, planes, n: int, ransac_n: int, probability: float = 0.99999999) -> np.ndarray:
    """Hypotheses whose Sigma|d| Open3D's selection can consult (o3dx_ransac_tied)."""
    c = _c(counts, np.int64)
    P = _c(planes, np.float64).reshape(-1, 4)
    out = np.zeros(max(len(c), 1), np.int32)
    k = np.zeros(1, np.int32)
    N.check(N.load().o3dx_ransac_tied(_np_ptr(c), _np_ptr(P), len(c), int(n), int(ransac_n), float(probability),
                                      _np_ptr(out), _np_ptr(k)), "ransac_tied")
    return out[: int(k[0])].copy()


def fx_to_double(fx) -> np.ndarray:
    """fx rows {lo, hi, q, 0} (int64, k x 4) -> float64 (k,), correctly rounded
    (o3dx_fx_to_double): the one conversion every path uses."""
    f = _c(fx, np.int64).reshape(-1, 4)
    out = np.zeros(max(len(f), 1), np.float64)
    N.check(N.load().o3dx_fx_to_double(_np_ptr(f), len(f), _np_ptr(out)), "fx_to_double")
    return out[: len(f)]


def absmax(xyz: torch.Tensor) -> np.ndarray:
    """|x|,|y|,|z| bounds of a cloud (from its AABB), float64 (3,)."""
    if xyz.shape[0] == 0:
        return np.zeros(3)
    mn, mx = aabb(xyz)
    return np.maximum(np.abs(mn), np.abs(mx))


def planes_from_samples(coords: np.ndarray, ransac_n: int) -> np.ndarray:
    """(H, ransac_n, 3) float64 sample coordinates -> (H, 4) planes
    (ComputeTrianglePlane / GetPlaneFromPoints, o3dx_planes_from_samples)."""
    c = _c(coords, np.float64).reshape(-1, ransac_n, 3)
    out = np.zeros((max(len(c), 1), 4), np.float64)
    N.check(N.load().o3dx_planes_from_samples(_np_ptr(c), len(c), int(ransac_n), _np_ptr(out)), "planes_from_samples")
    return out[: len(c)]


def plane_from_points(pts: np.ndarray) -> np.ndarray:
    p = _c(pts, np.float64).reshape(-1, 3)
    out = np.zeros(4, np.float64)
    N.check(N.load().o3dx_plane_from_points(_np_ptr(p), len(p), _np_ptr(out)), "plane_from_points")
    return out


def ransac_select(counts, sums, planes, n, ransac_n, probability=0.99999999) -> int:
    c = _c(counts, np.int64)
    s = _c(sums, np.float64)
    P = _c(planes, np.float64).reshape(-1, 4)
    return int(N.load().o3dx_ransac_select(_np_ptr(c), _np_ptr(s), _np_ptr(P), len(c), int(n), int(ransac_n),
                                           float(probability)))


def ransac_break_iteration(fitness: float, ransac_n: int, probability: float, num_iterations: int) -> int:
    """The selection replays' early-stop point for a new best fitness
    (o3dx_ransac_break_iteration): num_iterations where the quotient underflows."""
    return int(N.load().o3dx_ransac_break_iteration(float(fitness), int(ransac_n), float(probability),
                                                    int(num_iterations)))


def plane_inliers(xyz: torch.Tensor, plane, distance_threshold: float) -> torch.Tensor:
    x = _xyz(xyz)
    L = N.load()
    n = x.shape[0]
    pl = _c(plane, np.float64)
    idx = torch.empty(max(n, 1), dtype=torch.int32, device=x.device)
    k = np.zeros(1, np.int64)
    ws = N.workspace(2 * n + 65536, x.device)
    N.check(L.o3dx_plane_inliers(N.ptr(x), n, _np_ptr(pl), float(distance_threshold), N.ptr(idx), _np_ptr(k),
                                 N.ptr(ws), ws.numel(), N.stream_ptr(x.device)), "plane_inliers")
    return idx[: int(k[0])]


def _plane_pts(xyz: torch.Tensor):
    """(tensor, entry point) for the plane selection: float64 coordinates go to
    o3dx_plane_select_f64 unrounded, anything else as float32."""
    if isinstance(xyz, torch.Tensor) and xyz.dtype == torch.float64:
        N.require_device(xyz, "points")
        if xyz.ndim != 2 or xyz.shape[1] != 3:
            raise RuntimeError(f"points must have shape (n, 3), got {tuple(xyz.shape)}")
        return xyz.contiguous(), N.load().o3dx_plane_select_f64
    return _xyz(xyz), N.load().o3dx_plane_select


def plane_select(xyz: torch.Tensor, plane, thickness, invert: bool = False) -> torch.Tensor:
    """Ascending int32 device indices of the points within `thickness` of the
    plane (|s| < thickness, or thickness[0] < s < thickness[1] for a tuple),
    complemented with `invert`; s = distance2plane (reference PointCloud.py:
    278-290, 400-404).  o3dx_plane_select (float32 points) or
    o3dx_plane_select_f64 (float64 points)."""
    x, fn = _plane_pts(xyz)
    L = N.load()
    n = x.shape[0]
    pl = _c(plane, np.float64).reshape(4)
    band = isinstance(thickness, tuple)
    lo, hi = (float(thickness[0]), float(thickness[1])) if band else (0.0, float(thickness))
    idx = torch.empty(max(n, 1), dtype=torch.int32, device=x.device)
    k = np.zeros(1, np.int64)
    ws = N.workspace(int(L.o3dx_plane_select_workspace_bytes(n)), x.device)
    N.check(fn(N.ptr(x), n, _np_ptr(pl), int(band), lo, hi, int(bool(invert)), None, N.ptr(idx), _np_ptr(k),
               N.ptr(ws), ws.numel(), N.stream_ptr(x.device)), "plane_select")
    return idx[: int(k[0])]


def plane_distance(xyz: torch.Tensor, plane) -> torch.Tensor:
    """float64 signed distance of every point to the plane, in the order of the
    reference's distance2plane (PointCloud.py:400-404).  o3dx_plane_select(_f64)."""
    x, fn = _plane_pts(xyz)
    n = x.shape[0]
    pl = _c(plane, np.float64).reshape(4)
    out = torch.empty(n, dtype=torch.float64, device=x.device)
    N.check(fn(N.ptr(x), n, _np_ptr(pl), 0, 0.0, 0.0, 0, N.ptr(out), None, None, None, 0,
               N.stream_ptr(x.device)), "plane_distance")
    return out


def plane_moments(xyz: torch.Tensor, idx: Optional[torch.Tensor], centroid=None, absmax=None,
                  return_fx: bool = False):
    """GetPlaneFromPoints moments over idx (exact fx sums): {x,y,z} (pass 1) or
    centred {xx,xy,xz,yy,yz,zz} (pass 2, `centroid` given).  absmax: the
    cloud's |x|,|y|,|z| bounds fixing the fx quantum (a sharded cloud passes
    the global ones).  With return_fx also the (3|6, 4) fx rows."""
    x = _xyz(xyz)
    L = N.load()
    count = x.shape[0] if idx is None else idx.numel()
    c = None if centroid is None else _c(centroid, np.float64)
    am = None if absmax is None else _c(absmax, np.float64)
    out = np.zeros(6, np.float64)
    fx = np.zeros((6, 4), np.int64)
    ws = N.workspace(int(L.o3dx_plane_moments_workspace_bytes(count)), x.device, "moments")
    ii = None if idx is None else idx.to(torch.int32).contiguous()
    N.check(L.o3dx_plane_moments(N.ptr(x), N.ptr(ii), count, _np_ptr(c), _np_ptr(am), _np_ptr(out), _np_ptr(fx),
                                 N.ptr(ws), ws.numel(), N.stream_ptr(x.device)), "plane_moments")
    k = 6 if centroid is not None else 3
    return (out[:k], fx[:k]) if return_fx else out[:k]


def plane_from_moments(sum_xyz, count, centred) -> np.ndarray:
    out = np.zeros(4, np.float64)
    N.check(N.load().o3dx_plane_from_moments(_np_ptr(_c(sum_xyz, np.float64)), int(count),
                                             _np_ptr(_c(centred, np.float64)), _np_ptr(out)), "plane_from_moments")
    return out


def _estimation(estimation) -> int:
    """The library's constant of an estimation name (ValueError on anything else)."""
    try:
        return N.ICP_ESTIMATIONS[estimation]
    except (KeyError, TypeError):
        raise ValueError(f"unknown ICP estimation {estimation!r}: one of {sorted(N.ICP_ESTIMATIONS)}") from None


class ICPTarget:
    """Persistent target structure (grid of target points + normals) for ICP.
    tgt_normals=None builds a target without normals, which serves the
    point-to-point estimation only."""

    def __init__(self, tgt: torch.Tensor, tgt_normals: Optional[torch.Tensor] = None,
                 max_correspondence_distance: Optional[float] = None):
        if max_correspondence_distance is None:
            raise TypeError("ICPTarget: max_correspondence_distance is required")
        # float64 targets: a float64 grid (o3dx_icp_target_build_f64), float64 sources
        self.f64 = _is64(tgt)
        self.xyz = _xyz64(tgt, "target points") if self.f64 else _xyz(tgt, "target points")
        self.normals = None if tgt_normals is None else _xyz(tgt_normals.to(self.xyz.device), "target normals")
        if self.normals is not None and self.normals.shape[0] != self.xyz.shape[0]:
            raise RuntimeError("target normals must match target points")
        L = N.load()
        nt = self.xyz.shape[0]
        self.max_corr = float(max_correspondence_distance)
        wsb = L.o3dx_icp_target_f64_workspace_bytes if self.f64 else L.o3dx_icp_target_workspace_bytes
        self.ws = torch.empty(wsb(nt), dtype=torch.uint8, device=self.xyz.device)
        self.desc = np.zeros(N.ICP_DESC_LEN, np.float64)
        tail = (nt, self.max_corr, N.ptr(self.ws), self.ws.numel(), _np_ptr(self.desc),
                N.stream_ptr(self.xyz.device))
        if self.normals is None:
            build = L.o3dx_icp_target_build_points_f64 if self.f64 else L.o3dx_icp_target_build_points
            N.check(build(N.ptr(self.xyz), *tail), "icp_target_build_points")
        else:
            build = L.o3dx_icp_target_build_f64 if self.f64 else L.o3dx_icp_target_build
            N.check(build(N.ptr(self.xyz), N.ptr(self.normals), *tail), "icp_target_build")

    def accumulate(self, src: torch.Tensor, T: np.ndarray, want_corr: bool = False, absmax=None,
                   return_fx: bool = False, estimation: str = "point_to_plane"):
        """Transform + 1-NN + the estimation's moments: (sums[32], corr or None)
        (+ the (32, 4) int64 fx rows with return_fx).  `src` is (n,3) float32,
        or the (n,4) output of spatial_sort (faster).  absmax: |x|,|y|,|z|
        bounds of the WHOLE source (a sharded source passes the global ones);
        default: spatial_sort's record of them, else the library measures src.
        estimation "point_to_point": the anchored Umeyama moments
        (include/o3dx.h), for icp_update(..., estimation="point_to_point")."""
        est = _estimation(estimation)
        if self.f64:
            raise RuntimeError("ICPTarget.accumulate: float64 targets run the device loop (register)")
        sorted4 = src.ndim == 2 and src.shape[1] == 4
        if sorted4:
            N.require_device(src, "source points")
            s = src.float().contiguous()
        else:
            s = _xyz(src.to(self.xyz.device), "source points")
        if absmax is None:
            absmax = getattr(src, "absmax", None)
            of = getattr(src, "absmax_of", None)
            if absmax is None and of is not None:  # spatial_sort's cloud, measured on first use only
                absmax = src.absmax = _absmax(of)
        L = N.load()
        ns = s.shape[0]
        TT = _c(T, np.float64).reshape(4, 4)
        am = None if absmax is None else _c(absmax, np.float64).reshape(3)
        sums = np.zeros(N.ICP_NSUMS, np.float64)
        fx = np.zeros((N.ICP_NSUMS, 4), np.int64)
        corr = torch.empty((max(ns, 1), 2), dtype=torch.int32, device=s.device) if want_corr else None
        nc = np.zeros(1, np.int64)
        ws = N.workspace(L.o3dx_icp_accumulate_workspace_bytes(ns), s.device, "icp_acc")
        N.check(L.o3dx_icp_accumulate_est(N.ptr(s), ns, 1 if sorted4 else 0, N.ptr(self.ws), _np_ptr(self.desc),
                                          _np_ptr(TT), self.max_corr, _np_ptr(am),
                                          _np_ptr(sums), _np_ptr(fx), N.ptr(corr), _np_ptr(nc), est, N.ptr(ws),
                                          ws.numel(), N.stream_ptr(s.device)), "icp_accumulate")
        out = (sums, (corr[: int(nc[0])] if want_corr else None))
        return out + (fx,) if return_fx else out

    def register(self, src: torch.Tensor, init=None, max_iteration: int = 30, relative_fitness: float = 1e-6,
                 relative_rmse: float = 1e-6, absmax=None, want_corr: bool = False,
                 estimation: str = "point_to_plane", with_scaling: bool = False):
        """Open3D registration_icp onto this target with the whole loop on the
        device (o3dx_icp_register_est): each iteration's fused correspondence
        + moments pass, the solve and the convergence test are queued at once
        and the host waits once.  `src` as in accumulate (the (n,4)
        spatial_sort output is faster).  estimation: "point_to_plane" or
        "point_to_point" (Umeyama; with_scaling as Open3D's option).  ->
        dict(transformation, fitness, inlier_rmse[, correspondence_set])."""
        est = _estimation(estimation)
        sorted4 = src.ndim == 2 and src.shape[1] == 4
        if sorted4:
            N.require_device(src, "source points")
            # the index column's encoding follows the dtype (spatial_sort:
            # int32 bits in a float32 column; spatial_sort_f64: the index as a
            # double), so a cast would corrupt it: the sorted form must match
            want = torch.float64 if self.f64 else torch.float32
            if src.dtype != want:
                raise RuntimeError(f"ICPTarget.register: a {'float64' if self.f64 else 'float32'} target takes the "
                                   f"({'spatial_sort_f64' if self.f64 else 'spatial_sort'}) sorted source, got "
                                   f"{src.dtype}")
            s = src.contiguous()
        elif self.f64:
            s = _xyz64(src.to(self.xyz.device), "source points")
        else:
            s = _xyz(src.to(self.xyz.device), "source points")
        if absmax is None:
            absmax = getattr(src, "absmax", None)
        L = N.load()
        ns = s.shape[0]
        T0 = _c(np.eye(4) if init is None else init, np.float64).reshape(4, 4)
        am = None if absmax is None else _c(absmax, np.float64).reshape(3)
        T = np.zeros((4, 4), np.float64)
        fit, rm = np.zeros(1), np.zeros(1)
        corr = torch.empty((max(ns, 1), 2), dtype=torch.int32, device=s.device) if want_corr else None
        nc = np.zeros(1, np.int64)
        ws = N.workspace(L.o3dx_icp_accumulate_workspace_bytes(ns), s.device, "icp_acc")
        reg = L.o3dx_icp_register_est_f64 if self.f64 else L.o3dx_icp_register_est
        N.check(reg(N.ptr(s), ns, 1 if sorted4 else 0, N.ptr(self.ws), _np_ptr(self.desc), _np_ptr(T0),
                    int(max_iteration), float(relative_fitness), float(relative_rmse), self.max_corr, _np_ptr(am),
                    _np_ptr(T), _np_ptr(fit), _np_ptr(rm), N.ptr(corr), _np_ptr(nc), est, 1 if with_scaling else 0,
                    N.ptr(ws), ws.numel(), N.stream_ptr(s.device)), "icp_register")
        out = {"transformation": T, "fitness": float(fit[0]), "inlier_rmse": float(rm[0])}
        if want_corr:
            out["correspondence_set"] = corr[: int(nc[0])]
        return out


class ICPShardLoop:
    """One rank's side of the sharded device loop (o3dx_icp_shard_*,
    distributed.registration_icp_sharded): the state lives in the workspace;
    step() queues the rank's match + moments into a 64-int64 digit tensor,
    the caller all-reduces it, finish() queues the shared solve / update.
    Nothing here waits on the device except state() and resume()."""

    def __init__(self, src: torch.Tensor, absmax, max_correspondence_distance: float, init=None):
        sorted4 = src.ndim == 2 and src.shape[1] == 4
        if sorted4:
            N.require_device(src, "source points")
            if src.dtype != torch.float32:
                raise RuntimeError("ICPShardLoop: float32 sources (spatial_sort output or (n,3))")
            self.src = src.contiguous()
        else:
            self.src = _xyz(src, "source points")
        self.sorted4 = 1 if sorted4 else 0
        self.ns = int(self.src.shape[0])
        self.mc = float(max_correspondence_distance)
        self.dev = self.src.device
        L = N.load()
        self.L = L
        self.ws = torch.empty(int(L.o3dx_icp_accumulate_workspace_bytes(self.ns)), dtype=torch.uint8,
                              device=self.dev)
        T0 = _c(np.eye(4) if init is None else init, np.float64).reshape(4, 4)
        am = _c(absmax, np.float64).reshape(3)
        self.st = N.stream_ptr(self.dev)
        N.check(L.o3dx_icp_shard_begin(_np_ptr(T0), _np_ptr(am), self.mc, self.ns, N.ptr(self.ws), self.ws.numel(),
                                       self.st), "icp_shard_begin")

    def step(self, target, digits: torch.Tensor, use_prior: bool, widen: float = float("inf")):
        tws = None if target is None else N.ptr(target.ws)
        desc = None if target is None else _np_ptr(target.desc)
        N.check(self.L.o3dx_icp_shard_step(N.ptr(self.src), self.ns, self.sorted4, tws, desc, self.mc,
                                           1 if use_prior else 0, float(widen), N.ptr(digits), N.ptr(self.ws),
                                           self.ws.numel(), self.st), "icp_shard_step")

    def finish(self, digits: torch.Tensor, n_total: int, it: int, max_iteration: int, relative_fitness: float,
               relative_rmse: float, target=None, win: Optional[torch.Tensor] = None, widen: float = float("inf")):
        desc = None if target is None else _np_ptr(target.desc)
        world = 0 if win is None else int(win.shape[0])
        N.check(self.L.o3dx_icp_shard_finish(N.ptr(digits), int(n_total), int(it), int(max_iteration),
                                             float(relative_fitness), float(relative_rmse), self.mc, desc,
                                             None if win is None else N.ptr(win), world, float(widen), self.ns,
                                             N.ptr(self.ws), self.ws.numel(), self.st), "icp_shard_finish")

    def state(self):
        """(T, fitness, inlier_rmse, info {done, iterations applied, window stop}) — one host wait"""
        T = np.zeros((4, 4), np.float64)
        fit, rm = np.zeros(1), np.zeros(1)
        info = np.zeros(3, np.int32)
        N.check(self.L.o3dx_icp_shard_state(self.ns, N.ptr(self.ws), self.ws.numel(), _np_ptr(T), _np_ptr(fit),
                                            _np_ptr(rm), _np_ptr(info), self.st), "icp_shard_state")
        return T, float(fit[0]), float(rm[0]), info

    def resume(self):
        N.check(self.L.o3dx_icp_shard_resume(self.ns, N.ptr(self.ws), self.ws.numel(), self.st), "icp_shard_resume")


def spatial_sort_f64(xyz: torch.Tensor, target_occ: float = 8.0) -> torch.Tensor:
    """(n,4) float64 form of spatial_sort for float64 sources (x, y, z,
    original index), o3dx_spatial_sort_f64: ICPTarget.register's fast input
    on a float64 target."""
    x = _xyz64(xyz)
    L = N.load()
    n = x.shape[0]
    out = torch.empty((max(n, 1), 4), dtype=torch.float64, device=x.device)
    ws = N.workspace(L.o3dx_spatial_sort_f64_workspace_bytes(n), x.device, "sort")
    N.check(L.o3dx_spatial_sort_f64(N.ptr(x), n, float(target_occ), N.ptr(out), N.ptr(ws), ws.numel(),
                                    N.stream_ptr(x.device)), "spatial_sort_f64")
    return out[:n]


def spatial_sort(xyz: torch.Tensor, target_occ: float = 8.0) -> torch.Tensor:
    """(n,4) float32 copy of the cloud in a compact spatial order (8^3 blocks of
    grid cells, Morton order inside a block); column 3 holds the original
    int32 index bits (o3dx_spatial_sort_bounds).  The tensor carries
    `.absmax`, the cloud's |x|,|y|,|z| bounds from the sort's own bounds pass
    (the default fx quanta of ICPTarget.accumulate / register, which then
    skip their own measuring pass and host wait; a sharded source passes the
    global bounds instead), and `.absmax_of`, the cloud itself."""
    x = _xyz(xyz)
    L = N.load()
    n = x.shape[0]
    out = torch.empty((max(n, 1), 4), dtype=torch.float32, device=x.device)
    ws = N.workspace(L.o3dx_spatial_sort_workspace_bytes(n), x.device, "sort")
    am = np.zeros(3, np.float64)
    N.check(L.o3dx_spatial_sort_bounds(N.ptr(x), n, float(target_occ), N.ptr(out), _np_ptr(am), N.ptr(ws),
                                       ws.numel(), N.stream_ptr(x.device)), "spatial_sort")
    res = out[:n]
    res.absmax = am  # the sort's own bounds: ICP on it skips its absmax pass
    res.absmax_of = x
    return res


def icp_update(sums, T: np.ndarray, estimation: str = "point_to_plane", with_scaling: bool = False) -> np.ndarray:
    """T <- solve(sums) * T in the library's own float64 order (o3dx_icp_update_est)."""
    est = _estimation(estimation)
    TT = np.array(T, np.float64).reshape(4, 4).copy()
    rc = N.load().o3dx_icp_update_est(_np_ptr(_c(sums, np.float64)), est, 1 if with_scaling else 0, _np_ptr(TT))
    if rc < 0:  # 1 solved, 0 singular (identity update, as Open3D), < 0 a library error
        N.check(rc, "icp_update")
    return TT


def icp_solve_point_to_point(sums, with_scaling: bool = False, return_status: bool = False):
    """The Umeyama update (4x4) of point-to-point sums (o3dx_icp_solve_point_to_point);
    with return_status also 1 (solved) or 0 (the identity update)."""
    upd = np.zeros((4, 4), np.float64)
    rc = N.load().o3dx_icp_solve_point_to_point(_np_ptr(_c(sums, np.float64)), 1 if with_scaling else 0,
                                                _np_ptr(upd))
    if rc < 0:
        N.check(rc, "icp_solve_point_to_point")
    return (upd, rc) if return_status else upd


def icp_solve(sums) -> np.ndarray:
    upd = np.zeros((4, 4), np.float64)
    rc = N.load().o3dx_icp_solve_point_to_plane(_np_ptr(_c(sums, np.float64)), _np_ptr(upd))
    if rc < 0:
        N.check(rc, "icp_solve")
    return upd


def registration_icp(src: torch.Tensor, tgt: torch.Tensor, tgt_normals: Optional[torch.Tensor],
                     max_correspondence_distance: float, init=None, max_iteration: int = 30,
                     relative_fitness: float = 1e-6, relative_rmse: float = 1e-6, return_corr: bool = True,
                     estimation: str = "point_to_plane", with_scaling: bool = False):
    """Open3D registration_icp on one device with TransformationEstimationPointToPlane
    (the default here) or, estimation="point_to_point", TransformationEstimationPointToPoint(with_scaling),
    for which tgt_normals may be None.  A float64 source or target: both in
    float64 (o3dx_registration_icp_est_f64)."""
    est = _estimation(estimation)
    if tgt_normals is None and est != N.ICP_POINT_TO_POINT:
        raise RuntimeError("registration_icp: point-to-plane needs target normals")
    f64 = _is64(src) or _is64(tgt)
    cv = _xyz64 if f64 else _xyz
    s = cv(src, "source points")
    t = cv(tgt.to(s.device), "target points")
    tn = None if tgt_normals is None else _xyz(tgt_normals.to(s.device), "target normals")
    L = N.load()
    ns, nt = s.shape[0], t.shape[0]
    T0 = np.eye(4) if init is None else _c(init, np.float64).reshape(4, 4)
    T0 = _c(T0, np.float64)
    T = np.zeros((4, 4), np.float64)
    fit = np.zeros(1)
    rm = np.zeros(1)
    corr = torch.empty((max(ns, 1), 2), dtype=torch.int32, device=s.device) if return_corr else None
    nc = np.zeros(1, np.int64)
    tws = N.workspace((L.o3dx_icp_target_f64_workspace_bytes if f64 else L.o3dx_icp_target_workspace_bytes)(nt),
                      s.device, "icp_target")
    ws = N.workspace((L.o3dx_registration_icp_f64_workspace_bytes if f64 else
                      L.o3dx_registration_icp_workspace_bytes)(ns), s.device, "icp")
    fn = L.o3dx_registration_icp_est_f64 if f64 else L.o3dx_registration_icp_est
    rc = fn(N.ptr(s), ns, N.ptr(t), N.ptr(tn), nt, float(max_correspondence_distance), _np_ptr(T0),
            int(max_iteration), float(relative_fitness), float(relative_rmse), _np_ptr(T), _np_ptr(fit),
            _np_ptr(rm), N.ptr(corr), _np_ptr(nc), est, 1 if with_scaling else 0, N.ptr(tws), tws.numel(),
            N.ptr(ws), ws.numel(), N.stream_ptr(s.device))
    N.check(rc, "registration_icp")
    out = {"transformation": T, "fitness": float(fit[0]), "inlier_rmse": float(rm[0])}
    if return_corr:
        out["correspondence_set"] = corr[: int(nc[0])]
    return out


def evaluate_registration(src: torch.Tensor, tgt: torch.Tensor, max_correspondence_distance: float, transformation=None):
    """Open3D evaluate_registration (GetRegistrationResultAndCorrespondences):
    every source point's nearest target point within the distance under the
    given transformation — registration_icp's step at max_iteration = 0."""
    return registration_icp(src, tgt, None, max_correspondence_distance, init=transformation, max_iteration=0,
                            estimation="point_to_point")


# ------------------------------------------------ FPFH, matching, RANSAC on correspondences
FPFH_DIM = 33
_SPFH_ROW = 36


def fpfh(xyz: torch.Tensor, normals: torch.Tensor, mode: int = N.SEARCH_HYBRID, knn: int = 100, radius: float = 0.0,
         return_spfh: bool = False):
    """Open3D compute_fpfh_feature: (n, 33) float32 on the device (o3dx_fpfh;
    the neighbour lists are knn_search(xyz, xyz, mode, knn, radius)).  With
    return_spfh also the integer SPFH bin counts (n, 33) uint8 and the list
    lengths (n,) uint8.  ValueError for knn / max_nn above MAX_KNN,
    NotImplementedError for a radius search (unbounded lists)."""
    if int(mode) == N.SEARCH_RADIUS:
        raise NotImplementedError("fpfh: a radius search has unbounded neighbour lists; use KNN or Hybrid")
    if int(mode) not in (N.SEARCH_KNN, N.SEARCH_HYBRID):
        raise ValueError(f"fpfh: unknown search mode {mode}")
    if int(knn) > N.MAX_KNN or int(knn) < 1:
        raise ValueError(f"fpfh: knn / max_nn must be in 1..{N.MAX_KNN} (O3DX_MAX_KNN), got {knn}")
    if _is64(xyz):
        raise NotImplementedError("float64 points are outside fpfh (pass float32 values)")
    x = _xyz(xyz)
    nr = _xyz(normals.to(x.device), "normals")
    n = x.shape[0]
    if nr.shape[0] != n:
        raise RuntimeError(f"fpfh: {n} points but {nr.shape[0]} normals")
    L = N.load()
    dev = x.device
    out = torch.zeros((n, FPFH_DIM), dtype=torch.float32, device=dev)
    rows = torch.zeros((n, _SPFH_ROW), dtype=torch.uint8, device=dev) if return_spfh else None
    if n > 0:
        ws = N.workspace(L.o3dx_fpfh_workspace_bytes(n, int(knn)), dev)
        N.check(L.o3dx_fpfh(N.ptr(x), N.ptr(nr), n, int(mode), int(knn), float(radius), N.ptr(out), N.ptr(rows),
                            N.ptr(ws), ws.numel(), N.stream_ptr(dev)), "fpfh")
    if return_spfh:
        return out, rows[:, :FPFH_DIM], rows[:, FPFH_DIM]
    return out


def _feat(t: torch.Tensor, what: str) -> torch.Tensor:
    N.require_device(t, what)
    if t.ndim != 2 or t.shape[1] != FPFH_DIM:
        raise RuntimeError(f"{what} must have shape (n, {FPFH_DIM}), got {tuple(t.shape)}")
    return t.float().contiguous()


def feature_match(src_feat: torch.Tensor, tgt_feat: torch.Tensor, return_d2: bool = False):
    """For each source row (33 float32) the nearest target row's index (ns,)
    int32, the lowest index on a tie (o3dx_feature_match)."""
    a = _feat(src_feat, "source features")
    b = _feat(tgt_feat.to(a.device), "target features")
    ns, nt = a.shape[0], b.shape[0]
    dev = a.device
    idx = torch.empty(ns, dtype=torch.int32, device=dev)
    d2 = torch.empty(ns, dtype=torch.float32, device=dev) if return_d2 else None
    if ns > 0:
        if nt == 0:
            raise RuntimeError("feature_match: no target features")
        L = N.load()
        ws = N.workspace(L.o3dx_feature_match_workspace_bytes(ns, nt), dev)
        N.check(L.o3dx_feature_match(N.ptr(a), ns, N.ptr(b), nt, N.ptr(idx), N.ptr(d2), N.ptr(ws), ws.numel(),
                                     N.stream_ptr(dev)), "feature_match")
    return (idx, d2) if return_d2 else idx


def correspondences_from_features(src_feat: torch.Tensor, tgt_feat: torch.Tensor, mutual_filter: bool = False,
                                  mutual_consistency_ratio: float = 0.1) -> torch.Tensor:
    """Open3D CorrespondencesFromFeatures: (C, 2) int32 on the device,
    ascending in the source index — the forward pairs (i, j(i)); with
    mutual_filter those with i(j(i)) == i, unless fewer than
    mutual_consistency_ratio * ns of them are mutual (then the forward pairs)."""
    a = _feat(src_feat, "source features")
    b = _feat(tgt_feat.to(a.device), "target features")
    ns, nt = a.shape[0], b.shape[0]
    if ns == 0 or nt == 0:
        return torch.zeros((0, 2), dtype=torch.int32, device=a.device)
    fwd = feature_match(a, b)
    i = torch.arange(ns, dtype=torch.int32, device=a.device)
    pairs = torch.stack([i, fwd], dim=1)
    if not mutual_filter:
        return pairs
    back = feature_match(b, a)
    keep = back[fwd.long()] == i
    mutual = pairs[keep]
    if mutual.shape[0] < float(mutual_consistency_ratio) * ns:
        return pairs
    return mutual.contiguous()


def umeyama_from_samples(coords: np.ndarray) -> np.ndarray:
    """TransformationEstimationPointToPoint(False) of H samples at once, host
    only: coords (H, ransac_n, 2, 3) float64 (source point, target point) ->
    (H, 4, 4); the identity for a rank-deficient sample."""
    c = _c(coords, np.float64)
    if c.ndim != 4 or c.shape[2:] != (2, 3) or c.shape[1] < 1:
        raise RuntimeError(f"umeyama_from_samples: coords must be (H, ransac_n, 2, 3), got {c.shape}")
    H, rn = c.shape[0], c.shape[1]
    T = np.zeros((max(H, 1), 4, 4), np.float64)
    N.check(N.load().o3dx_umeyama_from_samples(_np_ptr(c), H, rn, _np_ptr(T)), "umeyama_from_samples")
    return T[:H]


def corr_check(coords: np.ndarray, T: np.ndarray, edge_similarity: float = -1.0,
               distance_threshold: float = -1.0) -> np.ndarray:
    """Open3D's correspondence checkers on H samples, host only (bool (H,)):
    EdgeLength(edge_similarity) and Distance(distance_threshold), each
    skipped when negative."""
    c = _c(coords, np.float64)
    H, rn = c.shape[0], c.shape[1]
    TT = _c(T, np.float64).reshape(-1, 4, 4)
    if TT.shape[0] != H:
        raise RuntimeError("corr_check: one transformation per sample")
    out = np.zeros(max(H, 1), np.uint8)
    N.check(N.load().o3dx_corr_check(_np_ptr(c), H, rn, _np_ptr(TT), float(edge_similarity),
                                     float(distance_threshold), _np_ptr(out)), "corr_check")
    return out[:H].astype(bool)


def _corr_inputs(src, tgt, corres):
    s = _xyz(src, "source points")
    t = _xyz(tgt.to(s.device), "target points")
    c = corres if isinstance(corres, torch.Tensor) else torch.as_tensor(np.asarray(corres).reshape(-1, 2))
    c = c.to(device=s.device, dtype=torch.int32).contiguous()
    if c.ndim != 2 or c.shape[1] != 2:
        raise RuntimeError(f"correspondences must have shape (C, 2), got {tuple(c.shape)}")
    if c.shape[0] > 0:
        lo = int(c.min().item())
        hi0, hi1 = int(c[:, 0].max().item()), int(c[:, 1].max().item())
        if lo < 0 or hi0 >= s.shape[0] or hi1 >= t.shape[0]:
            raise RuntimeError("correspondences: an index is out of range")
    return s, t, c


def _corr_call(name, src, tgt, corres, T, max_distance, want_sums):
    s, t, c = _corr_inputs(src, tgt, corres)
    TT = _c(T, np.float64).reshape(-1, 4, 4)
    H, C = TT.shape[0], c.shape[0]
    L = N.load()
    counts = np.zeros(max(H, 1), np.int64)
    ws = N.workspace(L.o3dx_corr_count_workspace_bytes(C, H), s.device)
    if want_sums:
        sums = np.zeros(max(H, 1), np.float64)
        N.check(L.o3dx_corr_error2(N.ptr(s), N.ptr(t), N.ptr(c), C, _np_ptr(TT), H, float(max_distance),
                                   _np_ptr(sums), _np_ptr(counts), N.ptr(ws), ws.numel(), N.stream_ptr(s.device)),
                name)
        return sums[:H], counts[:H]
    N.check(L.o3dx_corr_count(N.ptr(s), N.ptr(t), N.ptr(c), C, _np_ptr(TT), H, float(max_distance),
                              _np_ptr(counts), N.ptr(ws), ws.numel(), N.stream_ptr(s.device)), name)
    return counts[:H]


def corr_count(src, tgt, corres, T, max_distance: float) -> np.ndarray:
    """Exact inlier counts (H,) int64 of the transformations T (H, 4, 4)
    over the correspondences: |T p - q| < max_distance (o3dx_corr_count)."""
    return _corr_call("corr_count", src, tgt, corres, T, max_distance, False)


def corr_error2(src, tgt, corres, T, max_distance: float, return_counts: bool = False):
    """Sum of d^2 over the inliers of each transformation, fixed-order float64
    (o3dx_corr_error2)."""
    sums, counts = _corr_call("corr_error2", src, tgt, corres, T, max_distance, True)
    return (sums, counts) if return_counts else sums


def ransac_est_k(fitness: float, ransac_n: int, confidence: float) -> float:
    """Open3D's iteration estimate log(1 - confidence) / log(1 - fitness^n);
    0 at fitness 1, +inf where the denominator rounds to 0."""
    if fitness >= 1.0:
        return 0.0
    den = np.log(1.0 - fitness ** ransac_n)
    if den == 0.0:
        return float("inf")
    return float(np.log(1.0 - confidence) / den)


class CorrRansacReplay:
    """Open3D's sequential selection rule of RegistrationRANSACBasedOnCorrespondence
    over scored hypotheses, fed in iteration order: better = larger fitness,
    or equal fitness with a smaller rmse; an improvement lowers est_k.  The
    counts alone decide est_k (an rmse improvement leaves the fitness as it
    is), so `consults` can name beforehand the hypotheses whose sum d^2 the
    rule needs."""

    def __init__(self, C: int, ransac_n: int, max_iteration: int, confidence: float):
        self.C, self.rn, self.conf = int(C), int(ransac_n), float(confidence)
        self.max_iteration = int(max_iteration)
        self.est_k = float(max_iteration)
        self.best_count = 0
        self.best_err2 = None  # sum d^2 of the best (None: not needed yet)
        self.best_itr = -1
        self.best_T = np.eye(4)
        self.floor = 0  # the iteration after the last one that lowered est_k

    def stopped(self, itr: int) -> bool:
        return itr >= self.est_k

    def processed(self) -> int:
        """Iterations the loop runs before est_k stops it: the first itr >=
        est_k, which cannot precede the iteration after the one that set it."""
        if self.est_k >= self.max_iteration:
            return self.max_iteration
        return int(min(self.max_iteration, max(self.floor, np.ceil(self.est_k))))

    def consults(self, itrs, counts):
        """Positions in (itrs, counts) whose sum d^2 the rule consults when it
        is fed them in order (ties with the running best), and whether the
        incoming best's own sum is consulted."""
        est_k, bc = self.est_k, self.best_count
        need, need_best, cur = [], False, -1  # cur: position of the running best in this batch
        for p, (itr, c) in enumerate(zip(itrs, counts)):
            if itr >= est_k:
                break
            c = int(c)
            if c > bc:
                bc, cur = c, p
                est_k = min(est_k, ransac_est_k(c / self.C, self.rn, self.conf))
            elif c == bc and c > 0:
                need.append(p)
                if cur >= 0:
                    need.append(cur)
                else:
                    need_best = True
        return sorted(set(need)), need_best

    def feed(self, itr: int, count: int, T, err2=None) -> bool:
        """One scored hypothesis; err2 (sum d^2) is required on a tie.  False
        once est_k has stopped the loop."""
        if itr >= self.est_k:
            return False
        count = int(count)
        better = count > self.best_count
        if not better and count == self.best_count and count > 0:
            # equal fitness: rmse = sqrt(err2 / count), the same count on both sides
            better = np.sqrt(err2 / count) < np.sqrt(self.best_err2 / count)
        if better:
            self.best_count, self.best_err2, self.best_itr = count, err2, int(itr)
            self.best_T = np.array(T, np.float64).reshape(4, 4)
            k = ransac_est_k(count / self.C, self.rn, self.conf)
            if k < self.est_k:
                self.est_k, self.floor = k, int(itr) + 1
        return True


def registration_ransac_based_on_correspondence(src: torch.Tensor, tgt: torch.Tensor, corres,
                                                max_correspondence_distance: float, ransac_n: int = 3,
                                                edge_similarity: float = -1.0, distance_threshold: float = -1.0,
                                                max_iteration: int = 100000, confidence: float = 0.999,
                                                samples: Optional[np.ndarray] = None, seed: int = 0,
                                                round_size: int = 4096):
    """Open3D RegistrationRANSACBasedOnCorrespondence with
    TransformationEstimationPointToPoint(False), given the sample list
    (ransac_samples(C, ransac_n, max_iteration, seed) unless passed): rounds
    of round_size iterations — host Umeyama and checkers, one sweep for the
    exact inlier counts of the survivors, the sequential rule replayed on the
    host.  The result does not depend on round_size.  Returns the winning
    transformation, its iteration index (-1: none scored better than nothing),
    the number of iterations processed, the correspondence fitness and rmse."""
    s, t, c = _corr_inputs(src, tgt, corres)
    C = c.shape[0]
    if ransac_n < 3 or C < ransac_n or max_correspondence_distance <= 0.0:
        return {"transformation": np.eye(4), "best_iteration": -1, "processed": 0, "scored": 0, "corr_fitness": 0.0,
                "corr_rmse": 0.0}
    max_iteration = max(int(max_iteration), 0)
    if samples is None:
        samples = ransac_samples(C, ransac_n, max_iteration, seed)
    ch = c.cpu().numpy()
    ps = s.cpu().numpy().astype(np.float64)[ch[:, 0]]
    qt = t.cpu().numpy().astype(np.float64)[ch[:, 1]]
    return corr_ransac_rounds(
        ps, qt, samples, ransac_n, edge_similarity, distance_threshold, max_iteration, confidence, round_size,
        lambda T: corr_count(s, t, c, T, max_correspondence_distance),
        lambda T: corr_error2(s, t, c, T, max_correspondence_distance))


def corr_ransac_rounds(ps: np.ndarray, qt: np.ndarray, samples, ransac_n: int, edge_similarity: float,
                       distance_threshold: float, max_iteration: int, confidence: float, round_size: int,
                       count_fn, err2_fn):
    """The host side of registration_ransac_based_on_correspondence: ps, qt (C,
    3) float64 are the correspondences' source and target points; count_fn /
    err2_fn score a batch of transformations (H, 4, 4) -> (H,) (the GPU sweeps
    corr_count and corr_error2)."""
    C = len(ps)
    smp = _c(samples, np.int32).reshape(-1, ransac_n)[:max_iteration]
    max_iteration = smp.shape[0]
    rp = CorrRansacReplay(C, ransac_n, max_iteration, confidence)
    round_size = max(int(round_size), 1)
    scored = 0
    for r0 in range(0, max_iteration, round_size):
        if rp.stopped(r0):
            break
        sm = smp[r0:min(r0 + round_size, max_iteration)]
        coords = np.stack([ps[sm], qt[sm]], axis=2)  # (H, ransac_n, 2, 3)
        T = umeyama_from_samples(coords)
        surv = np.nonzero(corr_check(coords, T, edge_similarity, distance_threshold))[0]
        # hypotheses past est_k are never scored: est_k only falls
        surv = surv[r0 + surv < rp.est_k]
        if len(surv) == 0:
            continue
        itrs = r0 + surv
        Ts = T[surv]
        counts = count_fn(Ts)
        need, need_best = rp.consults(itrs, counts)
        Tq = [Ts[p] for p in need] + ([rp.best_T] if need_best and rp.best_err2 is None else [])
        err = {}
        if Tq:
            e2 = err2_fn(np.stack(Tq))
            err = {p: float(e2[k]) for k, p in enumerate(need)}
            if len(Tq) > len(need):
                rp.best_err2 = float(e2[len(need)])
        for p, itr in enumerate(itrs):
            if not rp.feed(int(itr), counts[p], Ts[p], err.get(p)):
                break
            scored += 1
    res = {"transformation": rp.best_T, "best_iteration": rp.best_itr, "processed": rp.processed(), "scored": scored,
           "corr_fitness": 0.0, "corr_rmse": 0.0}
    if rp.best_count > 0:
        if rp.best_err2 is None:
            rp.best_err2 = float(err2_fn(rp.best_T[None])[0])
        res["corr_fitness"] = rp.best_count / C
        res["corr_rmse"] = float(np.sqrt(rp.best_err2 / rp.best_count))
    return res


_absmax = absmax  # for ICPTarget.accumulate, whose parameter of that name shadows it


# ---------------------------------------------------------------- radius sweeps, ISS keypoints
def _sweep_points(xyz):
    f64 = _is64(xyz)
    return (_xyz64(xyz) if f64 else _xyz(xyz)), f64


def _check_radius(radius, what="radius"):
    radius = float(radius)
    if not np.isfinite(radius) or radius < 0.0:
        raise ValueError(f"{what} must be finite and >= 0, got {radius}")
    return radius


def radius_count(xyz: torch.Tensor, radius: float, cap=None) -> torch.Tensor:
    """|N_r(i)| per point (o3dx_radius_count): the number of points with
    d^2 < radius^2 (strict, the point itself included, float64 d^2), an (n,)
    int32 device tensor; with cap, min(count, cap) (the sweep stops there).
    float64 points: o3dx_radius_count_f64."""
    radius = _check_radius(radius)
    x, f64 = _sweep_points(xyz)
    n = x.shape[0]
    dev = x.device
    count = torch.zeros(n, dtype=torch.int32, device=dev)
    if n == 0 or radius == 0.0:  # d^2 < 0 holds for no pair
        return count
    L = N.load()
    wsb, fn = ((L.o3dx_radius_count_f64_workspace_bytes, L.o3dx_radius_count_f64) if f64 else
               (L.o3dx_radius_count_workspace_bytes, L.o3dx_radius_count))
    ws = N.workspace(wsb(n), dev)
    N.check(fn(N.ptr(x), n, radius, 0 if cap is None else max(int(cap), 1), N.ptr(count), N.ptr(ws), ws.numel(),
               N.stream_ptr(dev)), "radius_count")
    return count


def model_resolution(xyz: torch.Tensor) -> float:
    """Open3D's ComputeModelResolution: (the sum over the points of sqrt(d^2)
    to entry [1] of their 2-NN list, where there is one) / n.  The search is
    ops.knn_search; the float64 sum runs on the device in a fixed order
    (o3dx_nn_distance_sum), so the value is the same bits run to run."""
    x, _ = _sweep_points(xyz)
    n = x.shape[0]
    if n == 0:
        return 0.0
    _, d2, cnt = knn_search(x, x, mode=N.SEARCH_KNN, knn=2)
    d2 = d2.contiguous()
    cnt = cnt.contiguous()
    L = N.load()
    out = np.zeros(1, np.float64)
    ws = N.workspace(256, x.device)
    N.check(L.o3dx_nn_distance_sum(N.ptr(d2), N.ptr(cnt), n, int(d2.shape[1]), 1, _np_ptr(out), N.ptr(ws),
                                   ws.numel(), N.stream_ptr(x.device)), "model_resolution")
    return float(out[0]) / n


def iss_saliency(xyz: torch.Tensor, radius: float, gamma_21: float = 0.975, gamma_32: float = 0.975,
                 min_neighbors: int = 5):
    """(s (n,) float64, count (n,) int32) on the device: the ISS saliency and
    |N_radius(i)| of every point (o3dx_iss_saliency; include/o3dx.h states the
    rule).  float64 points: o3dx_iss_saliency_f64."""
    radius = _check_radius(radius)
    x, f64 = _sweep_points(xyz)
    n = x.shape[0]
    dev = x.device
    s = torch.zeros(n, dtype=torch.float64, device=dev)
    count = torch.zeros(n, dtype=torch.int32, device=dev)
    if n == 0 or radius == 0.0:
        return s, count
    L = N.load()
    wsb, fn = ((L.o3dx_iss_saliency_f64_workspace_bytes, L.o3dx_iss_saliency_f64) if f64 else
               (L.o3dx_iss_saliency_workspace_bytes, L.o3dx_iss_saliency))
    ws = N.workspace(wsb(n), dev)
    N.check(fn(N.ptr(x), n, radius, float(gamma_21), float(gamma_32), int(min_neighbors), N.ptr(s), N.ptr(count),
               N.ptr(ws), ws.numel(), N.stream_ptr(dev)), "iss_saliency")
    return s, count


def iss_nms(xyz: torch.Tensor, s: torch.Tensor, radius: float, min_neighbors: int = 5) -> torch.Tensor:
    """The ISS keypoints of a saliency (o3dx_iss_nms): ascending int32 device
    indices of the points with s > 0, at least min_neighbors points within
    radius and no neighbour of larger s.  float64 points: o3dx_iss_nms_f64."""
    radius = _check_radius(radius)
    x, f64 = _sweep_points(xyz)
    n = x.shape[0]
    dev = x.device
    if n == 0 or radius == 0.0:
        return torch.zeros(0, dtype=torch.int32, device=dev)
    N.require_device(s, "s")
    sv = s.to(torch.float64).contiguous()
    if sv.shape != (n,):
        raise RuntimeError(f"s must have shape ({n},), got {tuple(sv.shape)}")
    L = N.load()
    wsb, fn = ((L.o3dx_iss_nms_f64_workspace_bytes, L.o3dx_iss_nms_f64) if f64 else
               (L.o3dx_iss_nms_workspace_bytes, L.o3dx_iss_nms))
    ws = N.workspace(wsb(n), dev)
    idx = torch.empty(n, dtype=torch.int32, device=dev)
    cnt = np.zeros(1, np.int64)
    N.check(fn(N.ptr(x), n, N.ptr(sv), radius, int(min_neighbors), N.ptr(idx), _np_ptr(cnt), N.ptr(ws), ws.numel(),
               N.stream_ptr(dev)), "iss_nms")
    return idx[:int(cnt[0])]


def iss_keypoints(xyz: torch.Tensor, salient_radius: float = 0.0, non_max_radius: float = 0.0,
                  gamma_21: float = 0.975, gamma_32: float = 0.975, min_neighbors: int = 5):
    """o3d.geometry.keypoint.compute_iss_keypoints on the device: (idx,
    salient_radius, non_max_radius), idx the keypoints as ascending int32
    device indices and the radii as used (6 and 4 model resolutions when
    either is 0.0)."""
    salient_radius = _check_radius(salient_radius, "salient_radius")
    non_max_radius = _check_radius(non_max_radius, "non_max_radius")
    x, _ = _sweep_points(xyz)
    if salient_radius == 0.0 or non_max_radius == 0.0:
        res = model_resolution(x)
        salient_radius, non_max_radius = 6.0 * res, 4.0 * res
    s, _ = iss_saliency(x, salient_radius, gamma_21, gamma_32, min_neighbors)
    idx = iss_nms(x, s, non_max_radius, min_neighbors)
    return idx, salient_radius, non_max_radius
