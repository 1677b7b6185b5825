"""Inputs of the global-registration tests (FPFH, matcher, correspondence
scorer) shared by tests/golden/make_globalreg_golden.py, the CPU tests and the
GPU tests: the smallest shapes where each kernel can go wrong."""
from __future__ import annotations

import numpy as np

BUNNY_TGT_VOXEL, BUNNY_SRC_VOXEL = 0.005, 0.006
BUNNY_NORMALS_TGT, BUNNY_NORMALS_SRC = (0.01, 30), (0.012, 30)
BUNNY_FPFH = (0.025, 64)
BUNNY_MAX_DIST = 0.0075
BUNNY_EDGE = 0.9
BUNNY_SEED = 20241021
BUNNY_MAX_ITER = 100000


def axis_angle(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.radians(deg)
    return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)


def bunny_truth():
    T = np.eye(4)
    T[:3, :3] = axis_angle((1, 2, 3), 75.0)
    T[:3, 3] = (0.05, -0.12, 0.08)
    return T


def bunny_pair(bunny):
    """-> (source float32, target float32, T): the target is the bunny at
    voxel 0.005; the source the whole bunny moved by M = (75 deg about
    (1, 2, 3), t), rounded to float32, at voxel 0.006.  T = M^-1 maps the
    source onto the target."""
    from oracle.np_restate import voxel_down_sample

    b = np.asarray(bunny, np.float32)
    tgt = b[voxel_down_sample(b, BUNNY_TGT_VOXEL)]
    M = bunny_truth()
    moved = (b.astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
    src = moved[voxel_down_sample(moved, BUNNY_SRC_VOXEL)]
    return np.ascontiguousarray(src), np.ascontiguousarray(tgt), np.linalg.inv(M)


def pose_error(T, T_true):
    """(rotation error in degrees, translation error) of T against T_true."""
    E = np.asarray(T) @ np.linalg.inv(T_true)
    c = np.clip((np.trace(E[:3, :3]) - 1.0) * 0.5, -1.0, 1.0)
    return float(np.degrees(np.arccos(c))), float(np.linalg.norm(E[:3, 3]))


# ------------------------------------------------------------------ FPFH
def fpfh_cases():
    """name -> (points float32, normals float32, mode name, knn, radius)"""
    rng = np.random.default_rng(331)
    out = {}
    v = rng.standard_normal((300, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    out["sphere_knn16"] = (v.astype(np.float32), v.astype(np.float32), "knn", 16, 0.0)
    out["sphere_knn2"] = (v.astype(np.float32), v.astype(np.float32), "knn", 2, 0.0)
    out["sphere_knn64"] = (v.astype(np.float32), v.astype(np.float32), "knn", 64, 0.0)
    # bumpy height field, uneven list lengths under Hybrid
    xy = rng.uniform(0, 1, (400, 2)) ** 1.5
    z = 0.08 * np.sin(9 * xy[:, 0]) * np.cos(7 * xy[:, 1])
    gx = 0.72 * np.cos(9 * xy[:, 0]) * np.cos(7 * xy[:, 1])
    gy = -0.56 * np.sin(9 * xy[:, 0]) * np.sin(7 * xy[:, 1])
    nr = np.stack([-gx, -gy, np.ones_like(gx)], 1)
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    out["bumpy_hybrid"] = (np.column_stack([xy, z]).astype(np.float32), nr.astype(np.float32), "hybrid", 24, 0.12)
    # 32 x 32 lattice plane with equal normals + one column stacked along the
    # normal (dp parallel to n: |v| == 0)
    g = np.stack(np.meshgrid(np.arange(32), np.arange(32), indexing="ij"), -1).reshape(-1, 2) * 0.125
    lat = np.column_stack([g, np.zeros(len(g))])
    col = np.column_stack([np.full(6, 2.0), np.full(6, 2.0), 0.125 * np.arange(1, 7)])
    p = np.concatenate([lat, col]).astype(np.float32)
    nr = np.tile(np.float32([0, 0, 1]), (len(p), 1))
    out["lattice_column"] = (p, nr, "knn", 12, 0.0)
    # exact duplicate points (d == 0 pairs)
    p = rng.uniform(-1, 1, (200, 3)).astype(np.float32)
    p = np.concatenate([p, p[:40], p[:10]])
    nr = rng.standard_normal((len(p), 3))
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    out["duplicates"] = (p, nr.astype(np.float32), "knn", 10, 0.0)
    # isolated points under Hybrid (list length 1) among a dense patch
    p = np.concatenate([rng.uniform(0, 0.3, (150, 3)), 10.0 + 5.0 * np.arange(1, 8)[:, None] * np.ones((7, 3))])
    nr = rng.standard_normal((len(p), 3))
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    out["isolated_hybrid"] = (p.astype(np.float32), nr.astype(np.float32), "hybrid", 30, 0.1)
    for n in (0, 1, 2):
        q = rng.uniform(0, 1, (n, 3)).astype(np.float32)
        out[f"tiny{n}"] = (q, np.tile(np.float32([0, 0, 1]), (n, 1)), "knn", 4, 0.0)
    return out


def lists_of(points, mode, knn, radius):
    """The library's neighbour lists on the CPU (oracle.knn_search)."""
    from oracle import oracle as O

    p = np.asarray(points, np.float32)
    if len(p) == 0:
        return np.zeros((0, knn), np.int32), np.zeros((0, knn)), np.zeros(0, np.int32)
    return O.knn_search(p, p, O.KNN if mode == "knn" else O.HYBRID, knn, radius)


# ---------------------------------------------------------------- matcher
def match_cases():
    """name -> (source rows, target rows) float32 (n, 33)"""
    rng = np.random.default_rng(257130)
    a = (rng.gamma(0.7, 20.0, (257, 33))).astype(np.float32)
    b = (rng.gamma(0.7, 20.0, (130, 33))).astype(np.float32)
    out = {"random_257x130": (a, b)}
    bd = b.copy()
    bd[100:116] = bd[5:21]  # 16 planted bitwise duplicates: the lowest index wins
    ad = a.copy()
    ad[:16] = bd[5:21] + np.float32(0.25)  # rows whose nearest target is a duplicated one
    out["duplicates_257x130"] = (ad, bd)
    out["nt1"] = (a[:70], b[:1])
    out["ns0"] = (a[:0], b)
    out["wide_65x700"] = (a[:65], (rng.gamma(0.7, 20.0, (700, 33))).astype(np.float32))
    return out


# ----------------------------------------------------------------- scorer
def scorer_case(C, H, seed=0):
    """A source / target pair with C correspondences and H transformations
    (float64 (H, 4, 4)), some of them near the truth."""
    rng = np.random.default_rng(1000 * C + H + seed)
    ns, nt = C + 5, C + 9
    src = rng.uniform(-1, 1, (ns, 3)).astype(np.float32)
    M = np.eye(4)
    M[:3, :3] = axis_angle(rng.standard_normal(3), 40.0)
    M[:3, 3] = rng.uniform(-0.5, 0.5, 3)
    tgt = np.zeros((nt, 3), np.float32)
    ci = rng.permutation(ns)[:C]
    cj = rng.permutation(nt)[:C]
    moved = src[ci].astype(np.float64) @ M[:3, :3].T + M[:3, 3]
    tgt[cj] = (moved + rng.normal(0, 0.02, moved.shape)).astype(np.float32)
    corr = np.stack([ci, cj], 1).astype(np.int32)
    Ts = np.tile(M, (H, 1, 1))
    for h in range(H):
        D = np.eye(4)
        D[:3, :3] = axis_angle(rng.standard_normal(3), 0.0 if h == 0 else rng.uniform(0, 3.0))
        D[:3, 3] = 0.0 if h == 0 else rng.normal(0, 0.02, 3)
        Ts[h] = D @ M
    return src, tgt, corr, Ts


def exact_threshold_case():
    """Integer-valued points and translations: distances are exact.  Under the
    identity the pairs sit at d = 0, 3 (== max, not counted), 5 and 2."""
    src = np.float32([[0, 0, 0], [1, 2, 2], [4, 0, 3], [2, 0, 0], [7, 7, 7]])
    tgt = np.float32([[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]])
    corr = np.int32([[0, 0], [1, 1], [2, 2], [3, 3]])
    Ts = np.tile(np.eye(4), (3, 1, 1))
    Ts[1, :3, 3] = (0, 0, 1)   # d = 1, sqrt(1 + 4 + 9), sqrt(16 + 16), sqrt(4 + 1)
    Ts[2, :3, 3] = (-1, -2, -2)  # d = 3 (not counted), 0, sqrt(9 + 4 + 1), sqrt(1 + 4 + 4) = 3 (not counted)
    return src, tgt, corr, Ts, 3.0, np.int64([2, 2, 1])
