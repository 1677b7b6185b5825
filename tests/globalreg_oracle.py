"""numpy restatement of Open3D's ComputeFPFHFeature, CorrespondencesFromFeatures
and RegistrationRANSACBasedOnCorrespondence, as DESIGN.md §4.11 states them.
Open3D's source was not at hand when this was written: this file is the
definition the tests pin, not a port.  TEST INFRASTRUCTURE ONLY.

Everything is float64 on the float32 inputs, in the written operation order
(numpy does not contract a * b + c).  The neighbour lists are an input, in the
library's (d^2, index) order — oracle.knn_search supplies them on the CPU."""
from __future__ import annotations

import numpy as np

PI = np.pi


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def pair_features(p1, n1, p2, n2, diag=None):
    """(f0, f1, f2) of each pair, arrays (..., 3) float64 in."""
    with np.errstate(all="ignore"):
        dp = p2 - p1
        d = np.sqrt(dot3(dp, dp))
        zero = d == 0.0
        ds = np.where(zero, 1.0, d)
        a1 = dot3(n1, dp) / ds
        a2 = dot3(n2, dp) / ds
        c1, c2 = np.arccos(np.abs(a1)), np.arccos(np.abs(a2))
        swap = c1 > c2  # on the acos values; NaN -> False
        if diag is not None:
            live = ~zero
            same = np.abs(a1).view(np.int64) == np.abs(a2).view(np.int64)
            gap = np.abs(c1 - c2)[live & ~same]
            diag["acos_gap_min"] = float(gap.min()) if gap.size else np.inf
            diag["acos_equal_pairs"] = int((live & same).sum())
            diag["acos_arg_max"] = float(max(np.abs(a1)[live].max(initial=0.0), np.abs(a2)[live].max(initial=0.0)))
        sw = swap[..., None]
        m1 = np.where(sw, n2, n1)
        m2 = np.where(sw, n1, n2)
        dq = np.where(sw, -dp, dp)
        f2 = np.where(swap, -a2, a1)
        v = cross3(dq, m1)
        vn = np.sqrt(dot3(v, v))
        vz = vn == 0.0
        v = v / np.where(vz, 1.0, vn)[..., None]
        w = cross3(m1, v)
        f1 = dot3(v, m2)
        f0 = np.arctan2(dot3(w, m2), dot3(m1, m2))
        dead = zero | vz
        f0 = np.where(dead, 0.0, f0)
        f1 = np.where(dead, 0.0, f1)
        f2 = np.where(dead, 0.0, f2)
    return f0, f1, f2


def _bins(f0, f1, f2, diag=None):
    x0 = 11.0 * (f0 + PI) / (2.0 * PI)
    x1 = 11.0 * (f1 + 1.0) * 0.5
    x2 = 11.0 * (f2 + 1.0) * 0.5
    if diag is not None:
        e = np.inf
        for x in (x0, x1, x2):
            r = np.rint(x)
            inner = (r >= 1) & (r <= 10)  # edges 0 and 11 clamp to the same bin on either side
            if inner.any():
                e = min(e, float(np.abs(x - r)[inner].min()))
        diag["bin_edge_min"] = e
    cl = lambda x: np.clip(np.nan_to_num(np.floor(x), nan=0.0), 0, 10).astype(np.int64)  # noqa: E731
    return cl(x0), cl(x1), cl(x2)


def fpfh(points, normals, idx, d2, cnt, diag=None):
    """-> (feature (n, 33) float64 before the float32 rounding, SPFH bin counts
    (n, 33) int64, SPFH rows (n, 33) float64)."""
    p = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    nr = np.asarray(normals, np.float32).astype(np.float64).reshape(-1, 3)
    n = len(p)
    if n == 0:
        return np.zeros((0, 33)), np.zeros((0, 33), np.int64), np.zeros((0, 33))
    idx = np.asarray(idx).reshape(n, -1)
    d2 = np.asarray(d2, np.float64).reshape(n, -1)
    m = np.asarray(cnt).astype(np.int64).reshape(n)
    K = idx.shape[1] if n else 0
    counts = np.zeros((n, 33), np.int64)
    spfh = np.zeros((n, 33))
    out = np.zeros((n, 33))
    if n == 0 or K < 2:
        return out, counts, spfh
    pos = np.arange(K)[None, :]
    live = (pos >= 1) & (pos < m[:, None])
    ii, ll = np.nonzero(live)
    jj = idx[ii, ll]
    f0, f1, f2 = pair_features(p[ii], nr[ii], p[jj], nr[jj], diag)
    h0, h1, h2 = _bins(f0, f1, f2, diag)
    np.add.at(counts, (ii, h0), 1)
    np.add.at(counts, (ii, 11 + h1), 1)
    np.add.at(counts, (ii, 22 + h2), 1)
    # inc added count times, one addition after the other
    with np.errstate(all="ignore"):
        inc = np.where(m > 1, 100.0 / np.maximum(m - 1, 1), 0.0)
    steps = np.cumsum(np.repeat(inc[:, None], max(K, 2), axis=1), axis=1)  # steps[i, c - 1] = c additions
    steps = np.concatenate([np.zeros((n, 1)), steps], axis=1)
    spfh = np.take_along_axis(steps, counts, axis=1)
    acc = np.zeros((n, 33))
    s = np.zeros((n, 3))
    with np.errstate(all="ignore"):
        for pl in range(1, K):
            use = (pl < m) & (d2[:, pl] != 0.0)
            if not use.any():
                continue
            j = np.where(use, idx[:, pl], 0)
            val = spfh[j] / np.where(use, d2[:, pl], 1.0)[:, None]
            val = np.where(use[:, None], val, 0.0)
            acc += val
            for b in range(33):
                s[:, b // 11] += val[:, b]
        sc = np.where(s != 0.0, 100.0 / np.where(s != 0.0, s, 1.0), s)
    out = acc * np.repeat(sc, 11, axis=1) + spfh
    out[m <= 1] = 0.0
    return out, counts, spfh


def match(src_feat, tgt_feat, chunk=64):
    """float64 argmin over direct differences on the float32 rows (lowest
    index on a tie) -> (idx int32 (ns,), relative gap (ns,) between the best
    and the runner-up squared distance: 0 = an exact tie, inf for nt == 1)."""
    a = np.asarray(src_feat, np.float32).astype(np.float64)
    b = np.asarray(tgt_feat, np.float32).astype(np.float64)
    ns, nt = len(a), len(b)
    idx = np.zeros(ns, np.int32)
    gap = np.full(ns, np.inf)
    for r0 in range(0, ns, chunk):
        e = a[r0:r0 + chunk, None, :] - b[None, :, :]
        d = np.zeros(e.shape[:2])
        for c in range(e.shape[2]):
            d += e[:, :, c] * e[:, :, c]
        k = np.argmin(d, axis=1)  # first minimum
        idx[r0:r0 + chunk] = k
        if nt > 1:
            best = d[np.arange(len(k)), k]
            d[np.arange(len(k)), k] = np.inf
            second = d.min(axis=1)
            with np.errstate(all="ignore"):
                gap[r0:r0 + chunk] = np.where(second == best, 0.0, (second - best) / np.where(second > 0, second, 1.0))
    return idx, gap


def correspondences(src_feat, tgt_feat, mutual_filter=False, ratio=0.1):
    fwd, _ = match(src_feat, tgt_feat)
    ns = len(fwd)
    pairs = np.stack([np.arange(ns, dtype=np.int32), fwd], axis=1).astype(np.int32)
    if not mutual_filter or ns == 0:
        return pairs
    back, _ = match(tgt_feat, src_feat)
    mutual = pairs[back[fwd] == np.arange(ns)]
    return pairs if len(mutual) < ratio * ns else mutual


def umeyama(P, Q):
    """Eigen::umeyama(P, Q, with_scaling=false) of each sample: P, Q (H, k, 3)
    float64 -> (H, 4, 4), by numpy's SVD."""
    P = np.asarray(P, np.float64)
    Q = np.asarray(Q, np.float64)
    pm, qm = P.mean(axis=1), Q.mean(axis=1)
    cov = np.einsum("hki,hkj->hij", Q - qm[:, None], P - pm[:, None]) / P.shape[1]
    U, _, Vt = np.linalg.svd(cov)
    d = np.where(np.linalg.det(U) * np.linalg.det(Vt) < 0, -1.0, 1.0)
    S = np.zeros((len(P), 3, 3))
    S[:, 0, 0] = S[:, 1, 1] = 1.0
    S[:, 2, 2] = d
    R = U @ S @ Vt
    T = np.tile(np.eye(4), (len(P), 1, 1))
    T[:, :3, :3] = R
    T[:, :3, 3] = qm - np.einsum("hij,hj->hi", R, pm)
    return T


def transform_dist(T, p, q):
    """|T p - q| in the pinned order: T (4, 4) or (H, 4, 4); p, q (C, 3)."""
    T = np.asarray(T, np.float64)
    if T.ndim == 2:
        T = T[None]
    x, y, z = p[None, :, 0], p[None, :, 1], p[None, :, 2]
    dd = []
    for r in range(3):
        dd.append((((T[:, r, 0, None] * x + T[:, r, 1, None] * y) + T[:, r, 2, None] * z) + T[:, r, 3, None])
                  - q[None, :, r])
    return np.sqrt((dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2])


def check_edge_length(P, Q, s):
    """(H,) bool: CorrespondenceCheckerBasedOnEdgeLength(s) on samples P, Q (H, k, 3)."""
    ok = np.ones(len(P), bool)
    k = P.shape[1]
    for i in range(k):
        for j in range(i + 1, k):
            e = P[:, i] - P[:, j]
            f = Q[:, i] - Q[:, j]
            ds, dt = np.sqrt(dot3(e, e)), np.sqrt(dot3(f, f))
            ok &= ~((ds < dt * s) | (dt < ds * s))
    return ok


def check_distance(P, Q, T, t):
    ok = np.ones(len(P), bool)
    for k in range(P.shape[1]):
        ok &= ~(_dist_rows(T, P[:, k], Q[:, k]) > t)
    return ok


def _dist_rows(T, p, q):
    dd = []
    for r in range(3):
        dd.append((((T[:, r, 0] * p[:, 0] + T[:, r, 1] * p[:, 1]) + T[:, r, 2] * p[:, 2]) + T[:, r, 3]) - q[:, r])
    return np.sqrt((dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2])


def est_k_of(fitness, ransac_n, confidence):
    if fitness >= 1.0:
        return 0.0
    with np.errstate(all="ignore"):
        den = np.log(1.0 - fitness ** ransac_n)
        return np.inf if den == 0.0 else float(np.log(1.0 - confidence) / den)


def score(T, p, q, max_d):
    d = transform_dist(T, p, q)[0]
    inl = d < max_d
    cnt = int(inl.sum())
    e2 = 0.0
    for v in d[inl]:
        e2 += v * v
    return cnt, e2, d


def ransac(src, tgt, corres, samples, max_d, ransac_n=3, edge_s=None, dist_t=None, confidence=0.999, transforms=None):
    """The sequential rule, iterations in order, given the sample list.
    -> dict(T, best_iteration, processed, scored, count, err2, thr_gap_min).
    transforms: the (H, 4, 4) Umeyama results to use instead of numpy's SVD."""
    p = np.asarray(src, np.float32).astype(np.float64)[corres[:, 0]]
    q = np.asarray(tgt, np.float32).astype(np.float64)[corres[:, 1]]
    C = len(corres)
    samples = np.asarray(samples).reshape(-1, ransac_n)
    max_it = len(samples)
    P, Q = p[samples], q[samples]
    T = umeyama(P, Q) if transforms is None else np.asarray(transforms, np.float64)
    ok = np.ones(max_it, bool)
    if edge_s is not None:
        ok &= check_edge_length(P, Q, edge_s)
    if dist_t is not None:
        ok &= check_distance(P, Q, T, dist_t)
    est_k = float(max_it)
    best = dict(T=np.eye(4), best_iteration=-1, count=0, err2=0.0)
    scored, gap, processed = 0, np.inf, max_it
    for itr in range(max_it):
        if itr >= est_k:
            processed = itr
            break
        if not ok[itr]:
            continue
        cnt, e2, d = score(T[itr], p, q, max_d)
        scored += 1
        gap = min(gap, float(np.abs(d - max_d).min()))
        fit, bfit = cnt / C, best["count"] / C
        rm = np.sqrt(e2 / cnt) if cnt else 0.0
        brm = np.sqrt(best["err2"] / best["count"]) if best["count"] else 0.0
        if fit > bfit or (fit == bfit and rm < brm):
            best = dict(T=T[itr].copy(), best_iteration=itr, count=cnt, err2=e2)
            est_k = min(est_k, est_k_of(fit, ransac_n, confidence))
    best.update(processed=processed, scored=scored, thr_gap_min=gap)
    return best


def rotation_angle_deg(R):
    return float(np.degrees(np.arccos(np.clip((np.trace(R) - 1.0) * 0.5, -1.0, 1.0))))
