"""Ties, degenerate systems and tiny clouds for the ICP loops, with plain
reference loops (helpers only; the tests are test_icp_loop_cases.py on the
CPU and test_gpu_icp_loop_edges.py on the GPU).

A case is a target, its normals (or None), a source, the initial T and
max_correspondence_distance; float32 unless its name starts with "wide_".
Every cloud is deterministic (edge_clouds.cloud, synthetic and integer
arithmetic) and holds at most 12 288 points.

  lattice_tie ... lattice_s3   every edge_clouds.icp_cases() entry, its T as
                  init.  lattice_tie under point-to-plane has residual
                  exactly 0 (the normals point up, the source lies in the
                  target's layers): T stays init and every step decides the
                  same ties again, now from a prior.  lattice_at_r never has a
                  correspondence.
  dup_target      every target point twice, under two indices of a fixed
                  permutation of the doubled cloud: every query has an exact
                  tie at every step while the source moves.
  walk_in         box_surface target and source under a motion that leaves
                  fewer than 60 % of the source within the radius at first
                  and more than 90 % after 8 iterations: rows cross the radius
                  in both directions between steps.  walk_in_n<k>: its first
                  k source rows (below a wave, below a block, block counts
                  that are no multiple of 8).
  walk_slow       the same clouds a fraction of a millimetre apart: from the
                  second step on the updates are small enough for the skip
                  proof to keep matches, and under point-to-point the source
                  keeps sliding by 1e-4 or so a step, so matched rows drift out
                  of the radius while their margin would still keep them (the
                  d < r^2 test of the kept arm).
  wide_*          float64.  At edge_clouds.OFFSET (~4.6e6 m) Open3D's
                  point-to-plane system is ill-conditioned (see the comment
                  above test_gpu_f64.test_f64_icp), so these run point-to-plane
                  at max_iteration 0 only and loop point-to-point;
                  wide_walk_in and wide_lattice_walk sit at the 1e4 m offset of
                  the existing float64 ICP tests and run everything they have
                  normals for.

The reference loops share no code with the library's device path:
point-to-plane is oracle.registration_icp, point-to-point
test_icp_p2p_host.np_registration_icp_p2p over a brute-force 1-NN
(edge_clouds.brute_knn: the (d^2, index) minimum with d^2 < r^2 strict).
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import edge_clouds as E
from oracle import oracle as O
from open3dpypro import synthetic as S
from test_icp_p2p_host import np_registration_icp_p2p

Case = namedtuple("Case", "name tgt tn src init r wide plane_loops")

# estimation key -> (the library's estimation, with_scaling)
ESTS = {"plane": ("point_to_plane", False), "point": ("point_to_point", False), "scaled": ("point_to_point", True)}
MAX_IT = 8  # the largest max_iteration of the GPU tests
OFF_1E4 = np.array([12345.678, 23456.789, 98.765])
WALK_N = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1793, 2049)
WALK_SEED = 31
WIDE_TINY = ((1, 1), (1, 2), (1, 3), (2, 1), (3, 1), (3, 3))
WALK_R = 0.02
SLOW_MOTION = dict(angle_deg=0.02, axis=(1.0, 2.0, 3.0), t=(3e-4, -2e-4, 2e-4))
WALK_MOTION = dict(angle_deg=3.0, axis=(1.0, 2.0, 3.0), t=(0.04, -0.03, 0.02))


def _ro(a):
    return None if a is None else E._ro(a)


def _rot(src64, T):
    return E.transform_unfused(src64, T)


@functools.lru_cache(maxsize=None)
def _walk_clouds():
    tgt = S.box_surface(8192, WALK_SEED).numpy()
    tn = O.estimate_normals(tgt, O.KNN, 30).astype(np.float32)
    src = S.apply_transform(S.box_surface(4096, WALK_SEED + 1), S.rigid_transform(**WALK_MOTION)).numpy()
    return _ro(tgt), _ro(tn), _ro(src)


@functools.lru_cache(maxsize=None)
def _walk_slow_source():
    return _ro(S.apply_transform(S.box_surface(4096, WALK_SEED + 1), S.rigid_transform(**SLOW_MOTION)).numpy())


@functools.lru_cache(maxsize=None)
def _dup_clouds():
    n = 3000
    base = S.box_surface(n, 71).numpy()
    bn = O.estimate_normals(base, O.KNN, 30).astype(np.float32)
    # the copies of point i sit at two unrelated indices of the doubled cloud
    # (a permutation of the second copy, then one of the whole)
    q, p = E._perm(n, 7, 3), E._perm(2 * n)
    tgt = np.concatenate([base, base[q]])[p]
    tn = np.concatenate([bn, bn[q]])[p]
    jit = (S.uniform_cube(2000, 72) - 0.5) * 0.004
    src = S.apply_transform(S.box_surface(n, 71)[:2000] + jit, S.rigid_transform(0.4, (3, 1, 2), (0.003, -0.002, 0.001)))
    return _ro(tgt.astype(np.float32)), _ro(tn), _ro(src.numpy())


def _full_mantissa(p32, seed):
    """float64 coordinates that float32 cannot hold: the float32 cloud plus up to a micrometre."""
    i = np.arange(p32.size, dtype=np.int64)
    import torch

    u = S.uniform01_f64(torch.from_numpy(i), seed).numpy().reshape(p32.shape)
    return p32.astype(np.float64) + u * 1e-6


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case, in a fixed order."""
    out = {}
    for name, (tgt, tn, src, T, r) in E.icp_cases().items():
        out[name] = Case(name, tgt, _ro(tn), _ro(src), _ro(np.array(T, np.float64)), float(r), False, True)
    tgt, tn, src = _dup_clouds()
    out["dup_target"] = Case("dup_target", tgt, tn, src, _ro(np.eye(4)), 0.02, False, True)
    tgt, tn, src = _walk_clouds()
    for n in WALK_N:
        out[f"walk_in_n{n}"] = Case(f"walk_in_n{n}", tgt, tn, _ro(src[:n]), _ro(np.eye(4)), WALK_R, False, True)
    out["walk_in"] = Case("walk_in", tgt, tn, src, _ro(np.eye(4)), WALK_R, False, True)
    out["walk_slow"] = Case("walk_slow", tgt, tn, _walk_slow_source(), _ro(np.eye(4)), WALK_R, False, True)
    # ---- float64
    wl = E.cloud("wide_lattice")
    step = 2.0 ** -4
    up = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (len(wl), 1))
    out["wide_lattice_tie"] = Case("wide_lattice_tie", wl, _ro(up), _ro(wl[:400] + np.array([0.5 * step, 0.0, 0.0])),
                                   _ro(np.eye(4)), 0.75 * step, True, False)
    # 1 to 3 targets and sources at the ~4.6e6 m offset: source row i lies 20
    # micrometres around target row i % nt, moved by init's centimetres.  Only
    # the (nt, ns) whose reference update is a translation or a full-rank
    # rotation: two pairs, or three sources on two targets, leave the rotation
    # about their common axis to the SVD's null space, and a rotation by
    # radians about the coordinate origin carries a translation of ~4.6e6,
    # past the |T_ij| <= 1e3 condition of test_icp_loop_cases.
    shift = np.eye(4)
    shift[:3, 3] = (0.01, -0.02, 0.005)
    for nt, ns in WIDE_TINY:
        nm = f"wide_tiny_t{nt}_s{ns}"
        t = E.cloud(f"wide_tiny{nt}")
        s = t[np.arange(ns) % nt] + (E._u(ns, 300 + ns).astype(np.float64) - 0.5) * 4e-5 - shift[:3, 3]
        out[nm] = Case(nm, t, _ro(up[:nt]), _ro(s), _ro(shift), 0.05, True, False)
    # walk_in as a scan-sized box (x 32, the size of synthetic.las_scene) with
    # full-mantissa coordinates.  Its point-to-plane reference loop loses
    # fitness from a start below 0.5 (conditioned() is False): a property case.
    out["wide_walk_in"] = Case("wide_walk_in", _ro(_full_mantissa(tgt * np.float32(32.0), 81) + OFF_1E4), tn,
                               _ro(_full_mantissa(src * np.float32(32.0), 82) + OFF_1E4), _ro(np.eye(4)),
                               32.0 * WALK_R, True, True)
    # a float64 loop whose matches no rounding can flip: lattice points one
    # step apart, the source a few of them under a small motion about their
    # centre (full-mantissa coordinates), the radius below half a step
    lat = E.cloud("lattice3d").astype(np.float64)
    c = lat.mean(0)
    M = S.rigid_transform(1.5, (2, -1, 3), (0.11, -0.07, 0.05))
    ls = _rot(lat[::3] - c, M) + c + OFF_1E4
    out["wide_lattice_walk"] = Case("wide_lattice_walk", _ro(lat + OFF_1E4), None, _ro(ls), _ro(np.eye(4)), 0.45, True,
                                    True)
    return out


def names(wide=None):
    c = cases()
    return [n for n in c if wide is None or c[n].wide == wide]


def ests_of(name):
    """The estimation keys a case runs (no point-to-plane without normals)."""
    return tuple(e for e in ESTS if e != "plane" or cases()[name].tn is not None)


def max_its_of(name, est, max_its=(0, 1, 5)):
    """The max_iteration values of a (case, estimation): point-to-plane at the
    ill-conditioned offset runs no update."""
    return (0,) if est == "plane" and not cases()[name].plane_loops else tuple(max_its)


def combos(wide=None, loops=False):
    """(case, estimation key) pairs; loops=True: only those that run updates."""
    return [(n, e) for n in names(wide) for e in ests_of(n) if not loops or max_its_of(n, e) != (0,)]


# ------------------------------------------------------------- references
def top2(tgt, q, chunk=512):
    """brute_table(tgt, q, 2) — the two nearest targets of every query in
    (d^2, index) order with nanoflann's expression — by two argmin passes
    (the first minimum of a row is the lowest index at that d^2):
    test_icp_loop_cases.test_top2_equals_brute_table holds it to
    edge_clouds.brute_table."""
    x = np.asarray(tgt, np.float64).reshape(-1, 3)
    q = np.asarray(q, np.float64).reshape(-1, 3)
    n, nq = len(x), len(q)
    m = min(2, n)
    idx = np.empty((nq, m), np.int32)
    d2o = np.empty((nq, m), np.float64)
    xs = [np.ascontiguousarray(x[:, a])[None, :] for a in range(3)]
    acc, t = np.empty((chunk, n)), np.empty((chunk, n))
    for a in range(0, nq, chunk):
        k = min(chunk, nq - a)
        A, B = acc[:k], t[:k]
        np.subtract(q[a:a + k, 0, None], xs[0], out=A)
        np.multiply(A, A, out=A)
        for c in (1, 2):  # ((dx dx + dy dy) + dz dz)
            np.subtract(q[a:a + k, c, None], xs[c], out=B)
            np.multiply(B, B, out=B)
            np.add(A, B, out=A)
        rows = np.arange(k)
        for j in range(m):
            i = np.argmin(A, 1)
            idx[a:a + k, j] = i
            d2o[a:a + k, j] = A[rows, i]
            A[rows, i] = np.inf
    return idx, d2o


_TABLES = {}


def table_at(case, q):
    """top2 of the case's target for the query points q, computed once per (case, points)."""
    key = (case.name, q.tobytes())
    if key not in _TABLES:
        _TABLES[key] = top2(case.tgt, q)
    return _TABLES[key]


def brute_corr(case, T, src=None):
    """edge_clouds.brute_corr of the case (or of other source rows on its target) under T."""
    src = case.src if src is None else src
    idx, _, cnt = E.brute_knn(case.tgt, None, O.HYBRID, 1, case.r, table=table_at(case, _rot(src, T)))
    has = cnt > 0
    return np.stack([np.nonzero(has)[0], idx[has, 0].astype(np.int64)], 1)


def metrics_of(case, T, corr, src=None):
    """(fitness, rmse, sum of d^2) of a correspondence set under T, icp_metrics' 0 / 0 rule."""
    src = case.src if src is None else src
    if len(corr) == 0:
        return 0.0, 0.0, 0.0
    d = _rot(src, T)[corr[:, 0]] - np.asarray(case.tgt, np.float64)[corr[:, 1]]
    s = float(((d[:, 0] ** 2 + d[:, 1] ** 2) + d[:, 2] ** 2).sum())
    return len(corr) / len(src), float(np.sqrt(s / len(corr))), s


def _plane_reference(case, m):
    T, fit, rm, corr = O.registration_icp(case.src, case.tgt, case.tn, case.r, init=case.init, max_iteration=m,
                                          relative_fitness=0.0, relative_rmse=0.0)
    return T, corr.astype(np.int64).reshape(-1, 2), fit, rm


def _brute_knn1(case):
    """np_registration_icp_p2p's 1-NN by brute force (the runs with
    max_iteration 0 .. M walk the same points: table_at searches each once)."""
    def knn1(q):
        if not np.isfinite(q).all():  # a NaN update (Umeyama's scale of one pair): a tree search finds nothing
            return np.full(len(q), -1), np.full(len(q), np.inf)
        idx, d2, cnt = E.brute_knn(case.tgt, None, O.HYBRID, 1, case.r, table=table_at(case, np.ascontiguousarray(q)))
        return np.where(cnt > 0, idx[:, 0], -1), d2[:, 0]

    return knn1


@functools.lru_cache(maxsize=None)
def trajectory(name, est, M=MAX_IT):
    """[(T, corr (m,2) int64 by source row, fitness, rmse)] of the reference
    loop after 0, 1, ..., M iterations (no early stop)."""
    case = cases()[name]
    if est == "plane":
        return [_plane_reference(case, m) for m in range(M + 1)]
    knn1 = _brute_knn1(case)
    out = []
    with np.errstate(all="ignore"):
        for m in range(M + 1):
            T, fit, rm, corr = np_registration_icp_p2p(case.src, case.tgt, case.r, ESTS[est][1], init=case.init,
                                                       max_iteration=m, relative_fitness=0.0, relative_rmse=0.0,
                                                       knn1=knn1)
            out.append((T, corr.astype(np.int64).reshape(-1, 2), fit, rm))
    return out


def reference_defined(name, est):
    """False where the reference loop itself leaves the numbers: Eigen's
    umeyama divides by the source pairs' variance, 0 for a single pair (or
    pairs of one source point), so with_scaling gives a NaN update there —
    where the library keeps T (solve_update_p2p's non-finite arm, checked on
    the host in test_icp_loop_cases).  These combinations get the GPU
    property checks, whose references are brute force and the host loop."""
    return all(np.isfinite(t[0]).all() for t in trajectory(name, est))


def coord_scale(case):
    return max(1.0, float(np.abs(case.tgt).max()), float(np.abs(case.src).max()))


def margin_bar(case):
    """What a decided match must clear: 1e-7 of the coordinates' size."""
    return 1e-7 * coord_scale(case)


def margin_at(case, T):
    """(smallest positive gap, exact ties) of the case's source rows under T:
    the gap of a row is the runner-up's distance less the best's where the
    best lies within the radius, and |best distance - r|; rows with a gap of
    exactly 0 (two targets at one d^2, or d^2 == r^2) are exact ties, decided
    by index or by the strict <, and are counted apart."""
    r2 = case.r * case.r
    _, d2 = table_at(case, _rot(case.src, T))
    d = np.sqrt(d2)
    tie = d2[:, 0] == r2
    gaps = [np.abs(d[:, 0] - case.r)[~tie]]
    if d2.shape[1] > 1:
        inr = d2[:, 0] < r2
        t2 = inr & (d2[:, 0] == d2[:, 1])
        gaps.append((d[:, 1] - d[:, 0])[inr & ~t2])
        tie = tie | t2
    g = np.concatenate(gaps)
    return (float(g.min()) if len(g) else np.inf), int(tie.sum())


def decided_margin(name, est, M=MAX_IT):
    """margin_at for every iteration 0 .. M of the reference trajectory (a generator)."""
    case = cases()[name]
    return (margin_at(case, T) for T, _, _, _ in trajectory(name, est, M))


def conditioned(name, est, M=MAX_IT, bar=1e8):
    """Whether every update of the reference trajectory solves a full-rank
    system: point-to-plane, the 6x6 normal matrix of the correspondences with
    its columns scaled to unit size (condition number below `bar`);
    point-to-point, at least three pairs whose cross-covariance has rank 2
    (second singular value above 1/sqrt(bar) of the first).  Rank-deficient
    systems (a flat target with all normals up, 1 to 3 source points, several
    sources on one target) hang on rounding-noise pivots and get the property
    checks only."""
    case = cases()[name]
    for T, corr, _, _ in trajectory(name, est, M)[:-1]:
        if len(corr) < 3:
            return False
        p = _rot(case.src, T)[corr[:, 0]]
        if est == "plane":
            n = np.asarray(case.tn, np.float64)[corr[:, 1]]
            J = np.concatenate([np.cross(p, n), n], 1)
            A = J.T @ J
            s = np.sqrt(np.maximum(np.diag(A), 1e-300))
            if not np.linalg.cond(A / np.outer(s, s)) < bar:
                return False
        else:
            q = np.asarray(case.tgt, np.float64)[corr[:, 1]]
            sv = np.linalg.svd((q - q.mean(0)).T @ (p - p.mean(0)), compute_uv=False)
            if not sv[1] > sv[0] / np.sqrt(bar):
                return False
    return True


# (case, estimation) pairs compared with the reference loop at the project's
# ICP bars: every match of the reference trajectory decided by more than
# margin_bar and every update full-rank.  test_icp_loop_cases.test_class_table
# asserts that this table is what parity_rule gives.
_WALK_SMALL = tuple(f"walk_in_n{k}" for k in (63, 64, 65, 255, 256, 257))
PARITY = frozenset(
    [(n, e) for n in ("lattice_tie", "flat_off", "tiny_t3_s3", "lattice_s3", "wide_lattice_walk") for e in ("point", "scaled")]
    + [(n, e) for n in ("dup_target", "walk_in", "walk_slow") + _WALK_SMALL for e in ESTS]
    + [("walk_in_n1793", "point"), ("walk_in_n1793", "scaled"), ("walk_in_n2049", "plane"), ("walk_in_n2049", "point")])


def in_parity(name, est):
    return (name, est) in PARITY


def parity_rule(name, est):
    if max_its_of(name, est) == (0,) or not reference_defined(name, est):
        return False
    bar = margin_bar(cases()[name])
    return all(g > bar for g, _ in decided_margin(name, est)) and conditioned(name, est)


def kept_rows_leaving(name, est, M=MAX_IT, guard=2.2):
    """Per step k >= 2 of the reference trajectory, the source rows matched at
    step k - 1 whose nearest target is the same at step k but now at d^2 >=
    r^2, and whose runner-up at step k - 1 lay more than `guard` times the
    row's motion farther than the match: rows the skip proof's margin alone
    would keep.  [(k, rows, largest motion of any row)]"""
    case = cases()[name]
    r2 = case.r * case.r
    out, prev = [], None
    for k, (T, _, _, _) in enumerate(trajectory(name, est, M)):
        q = _rot(case.src, T)
        idx, d2 = table_at(case, q)
        if prev is not None and k >= 2:
            pq, pidx, pd2 = prev
            mot = np.sqrt(((q - pq) ** 2).sum(1))
            leave = (pd2[:, 0] < r2) & (d2[:, 0] >= r2) & (idx[:, 0] == pidx[:, 0])
            keep = (np.sqrt(pd2[:, 1]) - np.sqrt(pd2[:, 0])) > guard * mot
            out.append((k, np.nonzero(leave & keep)[0], float(mot.max())))
        prev = (q, idx, d2)
    return out


# ---------------------------------------------------------- planted priors
def _shift(x):
    T = np.eye(4)
    T[0, 3] = x
    return T


def prior_cases():
    """name -> (case name, source, T1, T2): a step under T1 plants its matches
    as the priors of a step under T2.  lat_low / lat_high: the lattice source
    0.25 (0.75) then 0.5 along x — the prior is the one (the other) member of
    the new tie; lat_far: the prior ends up far outside the radius, no match;
    walk: two unrelated small rigid motions about walk_in's aligned pose."""
    lat = E.cloud("lattice3d")[::4]  # rows from all over the index range: the x + 1 neighbour's index lies on either side
    walk = cases()["walk_in"].src
    back = np.linalg.inv(S.rigid_transform(**WALK_MOTION))  # walk_in's source roughly onto its target
    return {"lat_low": ("lattice_tie", lat, _shift(0.25), _shift(0.5)),
            "lat_high": ("lattice_tie", lat, _shift(0.75), _shift(0.5)),
            "lat_far": ("lattice_tie", lat, _shift(0.25), _shift(40.0)),
            "walk": ("walk_in", walk, S.rigid_transform(0.5, (0, 1, 0), (0.006, 0.0, -0.004)) @ back,
                     S.rigid_transform(0.4, (1, 2, 3), (-0.004, 0.006, 0.0)) @ back)}


@functools.lru_cache(maxsize=None)
def prior_normals(cname):
    """The target normals of the planted-prior steps: the case's own, except on
    the lattice, where every point gets another unit normal (all normals up
    would give both members of a tie the same moments)."""
    if cname != "lattice_tie":
        return cases()[cname].tn
    v = S.uniform_cube(len(cases()[cname].tgt), 91).numpy().astype(np.float64) * 2.0 - 1.0
    return _ro((v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32))


def prior_rows(name):
    """(prior target row per source row (-1: none), brute_table(2) under T2) of a planted-prior case."""
    cname, src, T1, T2 = prior_cases()[name]
    c = cases()[cname]
    idx, _, cnt = E.brute_knn(c.tgt, None, O.HYBRID, 1, c.r, table=table_at(c, _rot(src, T1)))
    return np.where(cnt > 0, idx[:, 0], -1), table_at(c, _rot(src, T2))


# ------------------------------------------------------------ shard splits
SHARD_CASES = ("lattice_tie", "lattice_at_r", "flat_off", "walk_in", "tiny_t3_s3")


def shard_splits(ns):
    """name -> row ranges [(a, b)] of a source of ns rows: 2 and 3 uneven
    shards, and 2 shards plus an empty one."""
    a, b = (ns + 2) // 3, ns - ns // 4
    if ns == 3:
        return {"two": [(0, 2), (2, 3)], "three": [(0, 1), (1, 2), (2, 3)], "empty": [(0, 2), (2, 3), (3, 3)]}
    return {"two": [(0, a), (a, ns)], "three": [(0, a), (a, b), (b, ns)], "empty": [(0, b), (b, b), (b, ns)]}
