"""numpy restatement of the radius sweeps: the neighbour count, the ISS saliency
and the ISS non-maximum suppression (o3d.geometry.keypoint.compute_iss_keypoints,
PointCloud.remove_radius_outlier).  Open3D's text is restated from memory; this
file is the definition the tests pin (include/o3dx.h states the same rules).

Neighbourhood: j is in N_r(i) when d^2(i,j) < r*r (strict, i itself included),
d^2 in float64 as ((dx*dx) + dy*dy) + dz*dz.  `neighbors_brute` is that rule by
chunked brute force; `neighbors` gives the same lists faster (a kd-tree proposes
the pairs within r * (1 + 1e-6), the same formula decides them) and falls back
to brute force without scipy.

Saliency: eigvalsh of the mean-centred covariance of the neighbours, cached per
neighbour set (keyed on the bytes of the ascending index list), so two points
with the same set get the same bits: the project's same-set rule.
"""
from __future__ import annotations

import numpy as np

TAU = 1e-9  # contested band, relative to e1 (see contested())


def _d2(q, p):
    """((dx*dx) + dy*dy) + dz*dz, float64, broadcasting over leading axes"""
    dx = q[..., 0] - p[..., 0]
    dy = q[..., 1] - p[..., 1]
    dz = q[..., 2] - p[..., 2]
    return ((dx * dx) + dy * dy) + dz * dz


def neighbors_brute(P, r, chunk=256):
    """CSR (indptr, indices) of N_r(i), ascending indices, by chunked brute force."""
    P = np.ascontiguousarray(P, np.float64)
    n = len(P)
    r2 = float(r) * float(r)
    ptr = [0]
    out = []
    for a in range(0, n, chunk):
        m = _d2(P[a:a + chunk, None, :], P[None, :, :]) < r2
        for row in m:
            idx = np.nonzero(row)[0]
            out.append(idx)
            ptr.append(ptr[-1] + len(idx))
    ind = np.concatenate(out) if out else np.zeros(0, np.int64)
    return np.asarray(ptr, np.int64), ind.astype(np.int64)


def neighbors(P, r):
    """neighbors_brute's lists; pairs proposed by a kd-tree when scipy is there."""
    P = np.ascontiguousarray(P, np.float64)
    n = len(P)
    try:
        from scipy.spatial import cKDTree
    except ImportError:  # pragma: no cover
        return neighbors_brute(P, r)
    if n == 0 or not (r > 0):
        return np.zeros(n + 1, np.int64), np.zeros(0, np.int64)
    scale = float(np.abs(P).max()) if n else 0.0
    rr = float(r) * (1.0 + 1e-6) + 64.0 * np.finfo(np.float64).eps * scale
    lists = cKDTree(P).query_ball_point(P, rr, return_sorted=True)
    ln = np.fromiter((len(x) for x in lists), np.int64, n)
    ind = np.concatenate([np.asarray(x, np.int64) for x in lists]) if n else np.zeros(0, np.int64)
    row = np.repeat(np.arange(n), ln)
    keep = _d2(P[row], P[ind]) < float(r) * float(r)
    ptr = np.zeros(n + 1, np.int64)
    np.add.at(ptr, row[keep] + 1, 1)
    return np.cumsum(ptr), ind[keep]


def counts(ptr):
    return np.diff(ptr).astype(np.int32)


def model_resolution(P):
    """(sum over the points, in index order, of sqrt(d^2) to entry [1] of the
    2-NN list sorted by (d^2, index), where the list has two entries) / n"""
    P = np.ascontiguousarray(P, np.float64)
    n = len(P)
    if n < 2:
        return 0.0
    second = np.empty(n, np.float64)
    try:
        from scipy.spatial import cKDTree

        k = min(n, 8)
        _, cand = cKDTree(P).query(P, k=k)
        d2 = np.sort(_d2(P[:, None, :], P[cand]), axis=1)
        second[:] = d2[:, 1]
    except ImportError:  # pragma: no cover
        for a in range(0, n, 256):
            d2 = np.sort(_d2(P[a:a + 256, None, :], P[None, :, :]), axis=1)
            second[a:a + 256] = d2[:, 1]
    total = 0.0
    for v in np.sqrt(second):  # the sequential sum
        total += float(v)
    return total / n


def saliency(P, ptr, ind, gamma_21, gamma_32, min_neighbors):
    """-> (s, e1, e2, e3), float64 per point; e* are 0 where the point is skipped"""
    P = np.ascontiguousarray(P, np.float64)
    n = len(P)
    s = np.zeros(n)
    e = np.zeros((n, 3))
    cache = {}
    for i in range(n):
        idx = ind[ptr[i]:ptr[i + 1]]
        k = len(idx)
        if k < min_neighbors or k == 0:
            continue
        key = idx.tobytes()
        hit = cache.get(key)
        if hit is None:
            Q = P[idx]
            D = Q - Q.mean(axis=0)
            C = D.T @ D / k
            if np.all(np.abs(C) <= 1e-12):  # Eigen's isZero()
                hit = (0.0, 0.0, 0.0, 0.0)
            else:
                w = np.linalg.eigvalsh(C)
                e1, e2, e3 = float(w[2]), float(w[1]), float(w[0])
                with np.errstate(divide="ignore", invalid="ignore"):
                    ok = bool(np.float64(e2) / np.float64(e1) < gamma_21) and \
                        bool(np.float64(e3) / np.float64(e2) < gamma_32)
                hit = (e3 if ok else 0.0, e1, e2, e3)
            cache[key] = hit
        s[i] = hit[0]
        e[i] = hit[1:]
    return s, e[:, 0], e[:, 1], e[:, 2]


def keypoints(s, ptr, ind, min_neighbors):
    """ascending int64 indices: s > 0, enough neighbours, no neighbour of larger s"""
    n = len(s)
    cnt = np.diff(ptr)
    row = np.repeat(np.arange(n), cnt)
    beaten = np.zeros(n, bool)
    np.logical_or.at(beaten, row, s[row] < s[ind])
    return np.nonzero((s > 0) & (cnt >= min_neighbors) & ~beaten)[0].astype(np.int64)


def contested(s, e1, e2, e3, ptr, ind, gamma_21, gamma_32, tau=TAU):
    """Points whose verdict a relative error of tau * e1 could change: an
    eigenvalue ratio on its gamma (a, b), a neighbour of nearly equal but
    different saliency (c), or a neighbour contested by (a, b) (d).

    tau: float64 moments of <= 10^3 terms about a common origin on clouds with
    extent / radius <= 40 carry a relative error of about n eps (L / r)^2 ~
    4e-10 of |C| at worst, the eigen solve a few eps |C|; tau sits above that
    and far below any real gap."""
    n = len(s)
    has = e1 > 0
    ab = has & ((np.abs(e2 - gamma_21 * e1) <= tau * e1) | (np.abs(e3 - gamma_32 * e2) <= tau * e1))
    row = np.repeat(np.arange(n), np.diff(ptr))
    si, sj = s[row], s[ind]
    close = (si != sj) & (np.abs(si - sj) <= tau * np.maximum(e1[row], e1[ind]))
    c = np.zeros(n, bool)
    np.logical_or.at(c, row, close)
    d = np.zeros(n, bool)
    np.logical_or.at(d, row, ab[ind])
    return ab | c | d


def iss(P, salient_radius=0.0, non_max_radius=0.0, gamma_21=0.975, gamma_32=0.975, min_neighbors=5):
    """The whole restatement: a dict of everything the tests compare."""
    P = np.ascontiguousarray(P, np.float64)
    n = len(P)
    res = None
    if salient_radius == 0.0 or non_max_radius == 0.0:
        res = model_resolution(P)
        salient_radius, non_max_radius = 6.0 * res, 4.0 * res
    if n == 0 or salient_radius == 0.0 or non_max_radius == 0.0:
        z = np.zeros(n)
        return dict(resolution=res, salient_radius=salient_radius, non_max_radius=non_max_radius, s=z, e1=z.copy(),
                    count=np.zeros(n, np.int32), count_nms=np.zeros(n, np.int32), contested=np.zeros(n, bool),
                    keypoints=np.zeros(0, np.int64))
    ptr, ind = neighbors(P, salient_radius)
    s, e1, e2, e3 = saliency(P, ptr, ind, gamma_21, gamma_32, min_neighbors)
    if non_max_radius == salient_radius:
        nptr, nind = ptr, ind
    else:
        nptr, nind = neighbors(P, non_max_radius)
    kp = keypoints(s, nptr, nind, min_neighbors)
    con = contested(s, e1, e2, e3, nptr, nind, gamma_21, gamma_32)
    return dict(resolution=res, salient_radius=salient_radius, non_max_radius=non_max_radius, s=s, e1=e1,
                count=counts(ptr), count_nms=counts(nptr), contested=con, keypoints=kp)


def same_set_pairs(ptr, ind):
    """(i, j) pairs, i < j consecutive members of each group of points with
    the same neighbour list"""
    groups = {}
    for i in range(len(ptr) - 1):
        groups.setdefault(ind[ptr[i]:ptr[i + 1]].tobytes(), []).append(i)
    out = []
    for g in groups.values():
        out.extend(zip(g[:-1], g[1:]))
    return np.asarray(out, np.int64).reshape(-1, 2)
