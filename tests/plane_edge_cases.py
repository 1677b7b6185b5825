"""Degenerate clouds and exact thresholds for RANSAC plane segmentation, with
plain references (helpers only; the tests are test_plane_edge_cases.py on the
CPU and test_gpu_plane_edges.py on the GPU).

A case is a cloud of edge_clouds (at most 12 288 points; float32 unless its
name starts with "wide_"), ransac_n, the hypotheses' samples, the threshold
and the probability.

  grid            every cloud of edge_clouds.names() with n >= ransac_n x
                  ransac_n (3, 5, 6) x H (1, 64, 300) x thr (0.01, 0.05, 1.0),
                  samples oracle.ransac_samples(n, ransac_n, H, 11); the clouds
                  at 1000.5 also at thr 1e-3, where the culled sweep's guard
                  sends segment_plane back to the dense sweep.
  lattice_at_thr  two lattice planes (z = 5 and x = 3) at a threshold exactly
                  one layer step, the float64 below it and the one above: the
                  neighbouring layers lie at |d| == thr and are out (strict <).
                  wide_lattice_at_thr: the same at 2^-4 on the georeferenced
                  lattice.
  degenerate_first  a repeated index and a collinear (or all-equal) triple
                  ahead of ordinary hypotheses: count -1, and the iteration
                  counter does not move (degenerate_counter: an early-stop
                  point of 1 that a counter moved by them would pass before
                  the best hypothesis comes).
  n_eq_rn         clouds of exactly ransac_n points (3, 4, 16), and H = 0.
  underflow       best fitness^ransac_n below 2^-53: the early-stop quotient
                  is -inf.

The references are written out in numpy float64 and share no code with
oracle/ (their agreement with it is asserted in test_plane_edge_cases.py):
the hypotheses' planes (ComputeTrianglePlane / GetPlaneFromPoints in their
own operation order), counts and sums with Open3D's predicate
|(a x + c z) + (b y + d)| < thr, the selection loop with its early stop, the
inliers and the refit.

The refit.  SegmentPlane refits with GetPlaneFromPoints, which is not the
total-least-squares plane: its normal is the column of the covariance's
adjugate (cofactor matrix) with the largest diagonal entry.  The adjugate of
C is sum_i (prod_{j != i} lambda_j) v_i v_i^T, so that column is a multiple
of the smallest eigenvector v_1 exactly when lambda_1 = 0 (the inliers
coplanar), and leans towards v_2 by about (lambda_1 / lambda_2) otherwise.
The eigenvector reference (numpy.linalg.eigh) is therefore the reference of
the refit only where the inliers are thin, lambda_1 <= THIN * lambda_2: there
it bounds the angle (eigh_bar); everywhere the plane is held to refit_o3d,
the same formula written out in numpy.  (On the CPU, seed 11: the oracle's
plane lies more than 1e-9 from the eigenvector plane in several hundred of
the conditioned cases, by up to 0.33 in a coefficient of the normal on the
tiny clouds at thr 1, where every point is an inlier; the eigenvector
reference binds 338 cases, test_class_table prints the count.)

Classes, decided from the references alone:
  selection pinned   the chosen hypothesis survives moving every Sigma|d|
                  by up to +-8 ulp (fixed generator, 16 trials), except the
                  sums that are the same bits in any order (order_free: no
                  terms, or lattice distances).  Unpinned cases get
                  inlier_property().
  refit conditioned  (lambda_2 - lambda_1) / lambda_3 >= 1e-6 over the
                  inliers' covariance, and the adjugate's largest diagonal
                  entry leads the next by 1e-6 of itself (adjugate_margin:
                  on a lattice diagonal two columns tie and rounding picks
                  the plane's sign), and one ulp of the centroid leaves the
                  normal within ATOL (centroid_resolved: not so for
                  micrometre inliers at the 4.6e6 m offset): the plane is
                  compared at ATOL = 1e-9 (assert_plane; on a wide_ cloud the
                  normal at ATOL and d as geometry, like
                  test_gpu_f64.test_f64_segment_plane: one ulp of d is 9.3e-10
                  there).  Otherwise plane_property(): unit normal,
                  d = -n . centroid, and a Rayleigh quotient n^T C n within
                  RAYLEIGH_MARGIN lambda_3 of lambda_1 (the measured margin,
                  below).
"""
from __future__ import annotations

import functools
import math
from collections import namedtuple

import numpy as np

import edge_clouds as E
from oracle import oracle as O

RN = (3, 5, 6)
HS = (1, 64, 300)
THRS = (0.01, 0.05, 1.0)
GUARD_THR = 1e-3
GUARD_CLOUDS = tuple(f"flat{a}@1000.5" for a in "xyz")
SEED = 11
PROB = 0.99999999
ATOL = 1e-9
GAP_BAR = 1e-6
PIN_ULPS, PIN_TRIALS = 8, 16
CAP_UNPINNED, CAP_UNCONDITIONED = 0.02, 0.10
THIN = 1e-9

# Measured on the CPU (seed 11; test_plane_edge_cases.test_class_table prints
# it and holds it to this figure): the largest excess of the oracle's own plane
# over the unconditioned cases, (n_ref^T C n_ref - lambda_1) / lambda_3, is
# 1.825e-3, at wide_collapsed-n5-H64-t0.05: the eight inliers are two sites
# 129 m apart, lambda_1 and lambda_2 (1e-12, the micrometres) are rounding
# noise next to lambda_3 = 6.7e3, so the adjugate is cancellation noise of the
# moments at the 4.6e6 m offset.  (Elsewhere the excess is below 5e-4: the lattice diagonals, whose
# three layers are not thin.)  Both sides solve one 3x3 problem in float64 and
# differ in how the moments were summed: the library gets 16 times the figure,
# and not less than 2^-40 (of lambda_3).
MEASURED_RAYLEIGH_EXCESS = 1.83e-3
RAYLEIGH_MARGIN = max(16.0 * MEASURED_RAYLEIGH_EXCESS, 2.0 ** -40)

Case = namedtuple("Case", "id cloud pts rn H thr samples prob wide kind")
Ref = namedtuple("Ref", "planes counts sums best tied consulted underflow inliers plane plane_eigh evals centroid cov "
                        "pinned conditioned")


def _rows(cloud, *pts):
    """Row indices of the given points in a cloud, looked up by value."""
    x = np.asarray(cloud, np.float64)
    out = []
    for p in pts:
        hit = np.nonzero((x == np.asarray(p, np.float64)).all(1))[0]
        assert len(hit) == 1, p
        out.append(int(hit[0]))
    return out


def _case(cid, cloud, rn, samples, thr, kind, pts=None, prob=PROB):
    pts = E.cloud(cloud) if pts is None else E._ro(pts)
    s = E._ro(np.asarray(samples, np.int32).reshape(-1, rn))
    return Case(cid, cloud, pts, rn, len(s), float(thr), s, prob, cloud.startswith("wide_"), kind)


@functools.lru_cache(maxsize=None)
def _samples(n, rn, H):
    return E._ro(O.ransac_samples(n, rn, H, SEED))


@functools.lru_cache(maxsize=None)
def cases():
    """id -> Case, in a fixed order."""
    out = {}

    def add(c):
        assert c.id not in out, c.id
        out[c.id] = c

    for name in E.names():
        n = len(E.cloud(name))
        for rn in RN:
            if n < rn:
                continue
            for H in HS:
                for thr in THRS + ((GUARD_THR,) if name in GUARD_CLOUDS else ()):
                    add(_case(f"{name}-n{rn}-H{H}-t{thr:g}", name, rn, _samples(n, rn, H), thr,
                              "guard" if thr == GUARD_THR else "grid"))
    # ---- lattice_at_thr
    lat = E.cloud("lattice3d")
    tri = [_rows(lat, (0, 0, 5), (1, 0, 5), (0, 1, 5)), _rows(lat, (3, 0, 0), (3, 4, 0), (3, 0, 7))]
    for tag, thr in (("at", 1.0), ("below", np.nextafter(1.0, 0.0)), ("above", np.nextafter(1.0, 2.0))):
        add(_case(f"lattice_at_thr-{tag}", "lattice3d", 3, tri, thr, "at_thr"))
    for tag, thr in (("at", 2.0 ** -4), ("above", np.nextafter(2.0 ** -4, 1.0))):
        add(_case(f"wide_lattice_at_thr-{tag}", "wide_lattice", 3, tri, thr, "at_thr"))
    # ---- degenerate_first
    for name in ("flatz@0", "flatx@1000.5", "lattice3d"):
        n = len(E.cloud(name))
        line = _rows(lat, (0, 0, 0), (1, 1, 1), (2, 2, 2)) if name == "lattice3d" else [7, 7, 7]
        s = np.concatenate([[[5, 5, 9], line, [4, 11, 4]], _samples(n, 3, 29)])
        add(_case(f"degenerate_first-{name}", name, 3, s, 0.05, "degenerate_first"))
    # the plane z = 1 (7 of 12 layers at thr 5.5: the early-stop point becomes
    # 1 at probability 0.25), two degenerate hypotheses, then z = 5 (11 of 12
    # layers), which the replay still consults, and one more that it does not
    s = [_rows(lat, (0, 0, 1), (1, 0, 1), (0, 1, 1)), [5, 5, 9], _rows(lat, (0, 0, 0), (1, 1, 1), (2, 2, 2)),
         tri[0], _rows(lat, (0, 0, 6), (1, 0, 6), (0, 1, 6))]
    add(_case("degenerate_counter", "lattice3d", 3, s, 5.5, "degenerate_first", prob=0.25))
    # ---- n == ransac_n
    for name, rn in (("tiny3", 3), ("tiny4", 4), ("tiny65", 16)):
        pts = E.cloud(name)[:rn]
        for H in (0, 1, 64):
            for thr in THRS:
                add(_case(f"n_eq_rn-{name}-n{rn}-H{H}-t{thr:g}", name, rn, _samples(rn, rn, H), thr, "n_eq_rn", pts=pts))
    # ---- underflow (the lattice3d / ransac_n 6 / thr 0.01 cases of the grid are the others)
    add(_case("underflow-tiny65-n16", "tiny65", 16, _samples(65, 16, 64), 0.01, "underflow"))
    return out


UNDERFLOW_GRID = tuple(f"lattice3d-n6-H{H}-t0.01" for H in HS)


def ids(cloud=None, wide=None, kind=None):
    return [c.id for c in cases().values()
            if (cloud is None or c.cloud == cloud) and (wide is None or c.wide == wide) and (kind is None or c.kind == kind)]


def clouds(wide=None):
    """The clouds that have cases, in a fixed order."""
    seen = {}
    for c in cases().values():
        if wide is None or c.wide == wide:
            seen.setdefault(c.cloud, None)
    return list(seen)


# ------------------------------------------------------------- references
def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _unit_plane(abc, c):
    """(abc / |abc|, -abc_unit . c), the zero plane where |abc| == 0; abc, c: 3 arrays of (H,)."""
    norm = np.sqrt(_dot(abc, abc))
    ok = norm != 0
    safe = np.where(ok, norm, 1.0)
    u = [a / safe for a in abc]
    pl = np.stack([u[0], u[1], u[2], -_dot(u, c)], -1)
    pl[~ok] = 0.0
    return pl


def _adjugate_normal(xx, xy, xz, yy, yz, zz):
    """GetPlaneFromPoints' normal before normalisation: the adjugate's column with the largest diagonal."""
    det_x, det_y, det_z = yy * zz - yz * yz, xx * zz - xz * xz, xx * yy - xy * xy
    cx = (det_x, xz * yz - xy * zz, xy * yz - xz * yy)
    cy = (xz * yz - xy * zz, det_y, xy * xz - yz * xx)
    cz = (xy * yz - xz * yy, xy * xz - yz * xx, det_z)
    fx = (det_x > det_y) & (det_x > det_z)
    fy = ~fx & (det_y > det_z)
    return [np.where(fx, cx[a], np.where(fy, cy[a], cz[a])) for a in range(3)]


def hyp_planes(p64, samples, rn):
    """(H, 4) hypothesis planes: ComputeTrianglePlane for ransac_n 3, else
    GetPlaneFromPoints over the sample in its order; zero = degenerate."""
    s = np.asarray(samples).reshape(-1, rn)
    if len(s) == 0:
        return np.zeros((0, 4))
    P = np.asarray(p64, np.float64)[s]  # (H, rn, 3)
    if rn == 3:
        e0 = [P[:, 1, a] - P[:, 0, a] for a in range(3)]
        e1 = [P[:, 2, a] - P[:, 0, a] for a in range(3)]
        abc = [e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]]
        return _unit_plane(abc, [P[:, 0, a] for a in range(3)])
    c = [np.zeros(len(s)) for _ in range(3)]
    for j in range(rn):
        for a in range(3):
            c[a] = c[a] + P[:, j, a]
    c = [v / float(rn) for v in c]
    m = {k: np.zeros(len(s)) for k in ("xx", "xy", "xz", "yy", "yz", "zz")}
    for j in range(rn):
        r = [P[:, j, a] - c[a] for a in range(3)]
        m["xx"] = m["xx"] + r[0] * r[0]
        m["xy"] = m["xy"] + r[0] * r[1]
        m["xz"] = m["xz"] + r[0] * r[2]
        m["yy"] = m["yy"] + r[1] * r[1]
        m["yz"] = m["yz"] + r[1] * r[2]
        m["zz"] = m["zz"] + r[2] * r[2]
    return _unit_plane(_adjugate_normal(m["xx"], m["xy"], m["xz"], m["yy"], m["yz"], m["zz"]), c)


def open3d_dist(p64, planes):
    """|(a x + c z) + (b y + d)| (n, H): Open3D's EvaluateRANSACBasedOnDistance
    expression in its own order, elementwise float64 (no fma)."""
    planes = np.asarray(planes, np.float64).reshape(-1, 4)
    a, b, c, d = (planes[:, k][None, :] for k in range(4))
    x, y, z = (np.asarray(p64, np.float64)[:, k][:, None] for k in range(3))
    return np.abs((a * x + c * z) + (b * y + d))


def open3d_counts(p64, planes, thr):
    """Inlier count of every plane under Open3D's predicate (degenerate planes not marked)."""
    return (open3d_dist(p64, planes) < thr).sum(0)


def counts_sums(p64, planes, thr):
    """(counts (H,) int64 with -1 at zero planes, Sigma|d| over the inliers (H,), 0 at zero planes)."""
    planes = np.asarray(planes, np.float64).reshape(-1, 4)
    if len(planes) == 0:
        return np.zeros(0, np.int64), np.zeros(0)
    d = open3d_dist(p64, planes)
    inl = d < thr
    counts = inl.sum(0).astype(np.int64)
    sums = np.where(inl, d, 0.0).sum(0)
    zero = ~np.any(planes != 0, 1)
    counts[zero] = -1
    sums[zero] = 0.0
    return counts, sums


def break_iteration(fit, rn, prob, H):
    """(early-stop point, whether fit^rn < 2^-53) for a new best fitness: 0 at
    fitness 1; a quotient log(1 - p) / log(1 - fit^rn) that is not >= 0 (the
    denominator is log(1) = 0 once fit^rn < 2^-53) means no early stop, H."""
    if fit >= 1.0:
        return 0, False
    pw = math.pow(fit, rn)
    num = math.log(1.0 - prob) if prob < 1.0 else -math.inf
    den = math.log(1.0 - pw)
    if den == 0.0:
        q = math.nan if num == 0.0 else -math.inf * (1.0 if num < 0 else -1.0)
    else:
        q = num / den
    under = pw < 2.0 ** -53
    if not q >= 0:
        return H, under
    return int(min(q, float(H))), under


Sel = namedtuple("Sel", "best tied consulted underflow")


def select(counts, sums, n, rn, prob=PROB):
    """Open3D's sequential selection with its early stop.  best: the chosen
    hypothesis (-1: none); tied: the hypotheses processed while their count
    equals the running maximum, for every maximum at least two of them reach
    (the only ones whose Sigma|d| can matter), ascending; consulted: every
    processed hypothesis with a positive count at or above the running
    maximum; underflow: whether an early-stop quotient underflowed."""
    H = len(counts)
    best, best_fit, best_rmse = -1, 0.0, 0.0
    brk, it, under = None, 0, False
    tied, run, consulted, top = [], [], [], 0
    for h in range(H):
        if brk is not None and it > brk:
            continue
        c = int(counts[h])
        if c < 0:
            continue
        fit = c / n if c else 0.0
        rmse = float(sums[h]) / math.sqrt(c) if c else 0.0
        if c > 0 and c >= top:
            consulted.append(h)
            if c > top:
                if len(run) >= 2:
                    tied += run
                run, top = [], c
            run.append(h)
        if fit > best_fit or (fit == best_fit and rmse < best_rmse):
            best, best_fit, best_rmse = h, fit, rmse
            brk, u = break_iteration(fit, rn, prob, H)
            under |= u
        it += 1
    if len(run) >= 2:
        tied += run
    return Sel(best, np.array(sorted(tied), np.int32), np.array(consulted, np.int32), under)


def covariance(p64, idx):
    """(centroid, centred covariance (3,3), eigenvalues ascending, eigenvectors) of the rows idx."""
    q = np.asarray(p64, np.float64)[idx]
    c = q.mean(0)
    r = q - c
    C = r.T @ r / len(q)
    w, v = np.linalg.eigh(C)
    return c, C, w, v


def refit_eigh(p64, idx):
    """The total-least-squares plane of the rows idx: the smallest eigenvector of their covariance."""
    c, _, _, v = covariance(p64, idx)
    nrm = v[:, 0]
    return np.array([nrm[0], nrm[1], nrm[2], -float(nrm @ c)])


def refit_o3d(p64, idx):
    """GetPlaneFromPoints of the rows idx in numpy: centroid, centred second
    moments (numpy's summation order), the adjugate column, normalised."""
    q = np.asarray(p64, np.float64)[idx]
    c = q.sum(0) / float(len(q))
    r = q - c
    xx, xy, xz = (r[:, 0] * r[:, 0]).sum(), (r[:, 0] * r[:, 1]).sum(), (r[:, 0] * r[:, 2]).sum()
    yy, yz, zz = (r[:, 1] * r[:, 1]).sum(), (r[:, 1] * r[:, 2]).sum(), (r[:, 2] * r[:, 2]).sum()
    abc = _adjugate_normal(*(np.array([v]) for v in (xx, xy, xz, yy, yz, zz)))
    return _unit_plane(abc, [np.array([v]) for v in c])[0]


def eigh_bar(evals):
    """How far GetPlaneFromPoints' normal may stand from the smallest
    eigenvector (sine of the angle) for thin inliers: the adjugate column is
    sum_i w_i v_i (v_i . e), w_1 = l2 l3, w_2 = l1 l3, w_3 = l1 l2, and its
    largest diagonal entry is at least a third of the trace, so the part
    outside v_1 is at most 3 (w_2 + w_3) / w_1 <= 6 l1 / l2 of it."""
    l1, l2, _ = (max(float(v), 0.0) for v in evals)
    return 6.0 * l1 / l2 + 1e-9 if l2 > 0 else np.inf


FREE_BITS = 40


def order_free(terms, thr):
    """Whether the sum of the non-negative float64 `terms` (all below thr) is
    the same bits however it is formed: all of them multiples of one power of
    two 2^q with the total below 2^53 quanta, so no partial sum rounds in any
    order, and 2^q no finer than 2^-FREE_BITS of thr's binade, so a
    fixed-point sum with that many bits below the threshold holds every term
    (lattice distances; no terms at all).  Rounding noise (one term of 1e-17
    under thr 0.01) is not order-free: its bits hang on how the sum is held."""
    t = np.asarray(terms, np.float64)
    t = t[t != 0]
    if len(t) == 0:
        return True
    m, e = np.frexp(t)
    mant = (m * 2.0 ** 53).astype(np.int64)
    low = int((e.astype(np.int64) - 53 + np.log2((mant & -mant).astype(np.float64)).astype(np.int64)).min())
    return math.fsum(t) / 2.0 ** low < 2.0 ** 53 and low >= math.frexp(thr)[1] - FREE_BITS


def pinned(counts, sums, n, rn, prob, best, free=None):
    """The chosen hypothesis survives +-PIN_ULPS ulp on every Sigma|d| that is not order-free (`free`)."""
    rng = np.random.default_rng(20240521)
    s = np.asarray(sums, np.float64)
    ulp = np.spacing(np.abs(s))
    if free is not None:
        ulp = np.where(free, 0.0, ulp)
    for _ in range(PIN_TRIALS):
        j = rng.integers(-PIN_ULPS, PIN_ULPS + 1, s.shape).astype(np.float64)
        if select(counts, s + j * ulp, n, rn, prob).best != best:
            return False
    return True


def adjugate_margin(p64, idx):
    """Relative lead of the largest diagonal entry of the covariance's adjugate
    over the runner-up: which column GetPlaneFromPoints takes, and with it the
    sign of the plane, hangs on rounding where this is ~0 (a lattice diagonal)."""
    q = np.asarray(p64, np.float64)[idx]
    r = q - q.mean(0)
    C = r.T @ r
    d = sorted([C[1, 1] * C[2, 2] - C[1, 2] ** 2, C[0, 0] * C[2, 2] - C[0, 2] ** 2, C[0, 0] * C[1, 1] - C[0, 1] ** 2])
    return (d[2] - d[1]) / d[2] if d[2] > 0 else 0.0


@functools.lru_cache(maxsize=None)
def reference(cid):
    """The Ref of a case (computed once)."""
    c = cases()[cid]
    p = np.asarray(c.pts, np.float64)
    n = len(p)
    planes = hyp_planes(p, c.samples, c.rn)
    counts, sums = counts_sums(p, planes, c.thr)
    sel = select(counts, sums, n, c.rn, c.prob)
    if sel.best < 0:
        inl = np.zeros(0, np.int64)
    else:
        inl = np.nonzero(open3d_dist(p, planes[sel.best])[:, 0] < c.thr)[0].astype(np.int64)
    if len(inl) == 0:
        z = np.zeros(3)
        return Ref(E._ro(planes), E._ro(counts), E._ro(sums), sel.best, sel.tied, sel.consulted, sel.underflow, inl,
                   np.zeros(4), np.zeros(4), z, z, np.zeros((3, 3)), True, True)
    cen, C, w, _ = covariance(p, inl)
    with np.errstate(all="ignore"):
        gap = (w[1] - w[0]) / w[2]
    # only the sums the replay can consult matter; which of them no order can change
    free = np.ones(len(sums), bool)
    if len(sel.tied):
        d = open3d_dist(p, planes[sel.tied])
        for j, h in enumerate(sel.tied):
            free[h] = order_free(d[d[:, j] < c.thr, j], c.thr)
    return Ref(E._ro(planes), E._ro(counts), E._ro(sums), sel.best, sel.tied, sel.consulted, sel.underflow, E._ro(inl),
               refit_o3d(p, inl), refit_eigh(p, inl), w, cen, C,
               pinned(counts, sums, n, c.rn, c.prob, sel.best, free),
               bool(gap >= GAP_BAR) and adjugate_margin(p, inl) >= GAP_BAR and centroid_resolved(cen, w))


def centroid_resolved(cen, evals):
    """Whether one ulp of the centroid leaves the normal within ATOL: a
    centroid moved by delta adds delta delta^T to the covariance, which turns
    the normal by about |delta|^2 / (lambda_2 - lambda_1).  False for
    micrometre inliers at the 4.6e6 m offset (ulp 9.3e-10), whose centroid the
    two sides round differently (one sum rounded once, a running sum)."""
    ulp = float(np.spacing(np.abs(cen).max()))
    return bool(ulp * ulp <= 0.1 * ATOL * (evals[1] - evals[0]))


# ---------------------------------------------------------------- checks
def inliers_of(cid, h):
    c = cases()[cid]
    return np.nonzero(open3d_dist(np.asarray(c.pts, np.float64), reference(cid).planes[h])[:, 0] < c.thr)[0]


def inlier_property(cid, inliers):
    """Selection unpinned: the inliers are those of some hypothesis whose count is the reference's best count."""
    r = reference(cid)
    top = r.counts[r.best]
    got = np.asarray(inliers, np.int64)
    assert len(got) == top, (cid, len(got), top)
    assert any(np.array_equal(got, inliers_of(cid, h)) for h in np.nonzero(r.counts == top)[0]), cid


def rayleigh(C, plane):
    nrm = np.asarray(plane, np.float64)[:3]
    return float(nrm @ C @ nrm)


def rank_deficient(evals):
    """Inliers on one line or in one point: lambda_2 is rounding noise next to lambda_3."""
    return not evals[1] > 1e-12 * evals[2]


def excess_over_lambda1(C, evals, plane):
    """(n^T C n - lambda_1) / lambda_3 (0 for coincident inliers)."""
    return (rayleigh(C, plane) - evals[0]) / evals[2] if evals[2] > 0 else 0.0


def plane_property(cid, plane, inliers=None):
    """Refit unconditioned: unit normal, d = -n . centroid to rounding, and a
    Rayleigh quotient n^T C n within RAYLEIGH_MARGIN lambda_3 of lambda_1.
    Where the inliers lie on a line or in a point GetPlaneFromPoints' adjugate
    is zero up to rounding, and the zero plane is an answer too."""
    c = cases()[cid]
    r = reference(cid)
    if inliers is None or np.array_equal(inliers, r.inliers):
        cen, C, w = r.centroid, r.cov, r.evals
    else:
        cen, C, w, _ = covariance(c.pts, np.asarray(inliers, np.int64))
    pl = np.asarray(plane, np.float64)
    assert np.isfinite(pl).all(), cid
    if not pl.any():
        assert rank_deficient(w), (cid, w)
        return
    assert abs(np.linalg.norm(pl[:3]) - 1.0) <= 1e-12, cid
    scale = max(1.0, float(np.abs(cen).max()))
    assert abs(pl[3] + float(pl[:3] @ cen)) <= 8 * np.spacing(scale), (cid, pl[3], float(pl[:3] @ cen))
    assert excess_over_lambda1(C, w, pl) <= RAYLEIGH_MARGIN, (cid, excess_over_lambda1(C, w, pl), w)


def assert_plane(cid, plane):
    """The plane of a conditioned case against the reference refit: every
    coefficient at ATOL on a float32 cloud.  On a wide_ cloud d = -n . c
    carries |c| ~ 4.6e6 (one ulp: 9.3e-10) times any change of n, so there the
    normal is held to ATOL and the planes' offsets to each other at the
    inliers' centroid, within ATOL + 8 ulp of the largest coordinate."""
    r = reference(cid)
    pl = np.asarray(plane, np.float64)
    if not cases()[cid].wide:
        np.testing.assert_allclose(pl, r.plane, rtol=0, atol=ATOL, err_msg=cid)
        return
    np.testing.assert_allclose(pl[:3], r.plane[:3], rtol=0, atol=ATOL, err_msg=cid)
    cen = r.centroid

    def off(q):
        return (q[0] * cen[0] + q[2] * cen[2]) + (q[1] * cen[1] + q[3])

    assert abs(off(pl) - off(r.plane)) <= ATOL + 8 * np.spacing(float(np.abs(cen).max())), (cid, off(pl), off(r.plane))


def eigh_applies(cid):
    """Whether the eigenvector reference binds the refit of a case: conditioned and thin inliers."""
    r = reference(cid)
    return bool(len(r.inliers)) and r.conditioned and r.evals[0] <= THIN * r.evals[1]


def assert_eigh(cid, plane):
    """The plane's normal against the smallest eigenvector of the inliers' covariance (sine of the angle, eigh_bar)."""
    r = reference(cid)
    s = float(np.linalg.norm(np.cross(np.asarray(plane, np.float64)[:3], r.plane_eigh[:3])))
    assert s <= eigh_bar(r.evals), (cid, s, eigh_bar(r.evals))


def check_result(cid, plane, inliers):
    """A segment_plane result of the case against its reference, by class."""
    r = reference(cid)
    plane = np.asarray(plane, np.float64)
    inliers = np.asarray(inliers, np.int64)
    if len(r.inliers) == 0:
        assert len(inliers) == 0 and np.array_equal(plane, np.zeros(4)), (cid, plane, len(inliers))
        return
    same = np.array_equal(inliers, r.inliers)
    if r.pinned:
        assert same, (cid, len(inliers), len(r.inliers))
    else:
        inlier_property(cid, inliers)
    if r.conditioned and same:
        assert_plane(cid, plane)
        if eigh_applies(cid):
            assert_eigh(cid, plane)
    else:
        plane_property(cid, plane, inliers)
