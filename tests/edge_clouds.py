"""Degenerate and tiny clouds for the neighbour search, with plain references
(helpers only; the tests are test_edge_clouds.py on the CPU and
test_gpu_edges.py on the GPU).

The clouds are deterministic (synthetic.uniform01 and integer arithmetic),
float32 unless their name starts with "wide_", and none holds more than
12 288 points: clouds lying exactly in an axis-aligned plane, on a line or in
one point (a search grid one cell thick), integer lattices (exact non-zero
distance ties at every k), two clusters far apart, a dense patch on a flat
cloud (the nested grid on a flat grid), float64 clouds at a georeferenced
offset, one of which the float32 search frame collapses.

The references are written out in numpy float64 and share no code with
oracle/ (their agreement with it is asserted in test_edge_clouds.py), except
FastEigen3x3 itself, taken from the oracle.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import oracle as O
from open3dpypro import synthetic as S

K = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)
K_COLLAPSED = (4, 5, 8, 30, 33)
TINY_N = (1, 2, 3, 4, 63, 64, 65, 255, 256, 257)
OFFSET = np.array([4.2e5, 4.6e6, 310.0])
FLAT = tuple(f"flat{a}@{c}" for a in "xyz" for c in ("0", "1000.5"))
# flat_nested's patch (test_edge_clouds.test_flat_nested_enters_the_nested_grid shows that its cells are dense)
PATCH_ORIGIN, PATCH_SIDE = (0.3, 0.7), 0.02


def _ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _u(n, seed):
    return S.uniform_cube(n, seed).numpy().copy()


def _perm(n, mul=1013, add=17):
    """A fixed permutation of range(n) (mul is prime and divides no n used here)."""
    p = (np.arange(n, dtype=np.int64) * mul + add) % n
    assert len(np.unique(p)) == n
    return p


def _lattice(nx, ny, nz):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    return g[_perm(len(g))].astype(np.float32)


@functools.lru_cache(maxsize=None)
def cloud(name: str) -> np.ndarray:
    """The cloud `name` (see names()), read-only."""
    if name.startswith("wide_"):
        return _ro(_wide(name))
    if name.startswith("tiny"):
        n = int(name[4:])
        return _ro(_u(n, 100 + n))
    if name == "same":
        return _ro(np.tile(_u(1, 7), (100, 1)))
    if name.startswith("flat") and "@" in name:
        axis, c = "xyz".index(name[4]), np.float32(float(name.split("@")[1]))
        p = _u(2000, 20 + axis)
        p[:, axis] = c
        return _ro(p)
    if name == "line_x":
        p = _u(500, 31)
        p[:, 1:] = 0.0
        return _ro(p)
    if name == "lattice3d":
        return _ro(_lattice(12, 12, 12))
    if name == "lattice2d":
        return _ro(_lattice(40, 40, 1))
    if name == "two_far":
        a = _u(1000, 41) * np.float32(0.01)
        b = _u(1000, 42) * np.float32(0.01) + np.array([1000.0, 0.0, 0.0], np.float32)
        return _ro(np.concatenate([a, b]).astype(np.float32))
    if name == "flat_nested":
        p = _u(8192, 51)
        d = _u(4096, 52) * np.float32(PATCH_SIDE)
        d[:, 0] += np.float32(PATCH_ORIGIN[0])
        d[:, 1] += np.float32(PATCH_ORIGIN[1])
        p = np.concatenate([p, d]).astype(np.float32)
        p[:, 2] = 0.25
        return _ro(p)
    raise KeyError(name)


def _wide(name):
    if name == "wide_flatz":
        return cloud("flatz@0").astype(np.float64) + OFFSET
    if name == "wide_lattice":
        return cloud("lattice3d").astype(np.float64) * 2.0 ** -4 + OFFSET  # exact: the ties survive
    if name.startswith("wide_tiny"):
        return cloud(name[5:]).astype(np.float64) + OFFSET
    if name == "wide_collapsed":
        # 1 500 sites x 4 points: the site, and the site moved by 1, 2 and 3
        # micrometres along x, y and z.  The sites lie on a 2^-10 m raster in
        # [64, 1000) m of the cloud's minimum corner, which one anchor point
        # (the last row) holds: the search frame is float32(p - min bound), and
        # float32 resolves a micrometre below 64 m, so without the anchor the
        # sites next to the minimum faces would not collapse.
        u = S.uniform_cube(1500, 61).numpy().astype(np.float64)
        site = 64.0 + np.floor(u * (936.0 * 1024.0)) / 1024.0
        disp = 1e-6 * np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 3]], np.float64)
        p = (site[:, None, :] + disp[None, :, :]).reshape(-1, 3)
        p = np.concatenate([p, np.zeros((1, 3))]) + OFFSET
        prox = (p - p.min(0)).astype(np.float32)[:-1].reshape(1500, 4, 3)
        assert (prox == prox[:, :1]).all(), "wide_collapsed: a float32 proxy resolves a displacement"
        assert len(np.unique(p, axis=0)) == len(p), "wide_collapsed: float64 points coincide"
        return p
    raise KeyError(name)


def names(wide=None):
    """Every cloud's name; wide=False / True: the float32 / float64 ones only."""
    f32 = [f"tiny{n}" for n in TINY_N] + ["same", *FLAT, "line_x", "lattice3d", "lattice2d", "two_far", "flat_nested"]
    f64 = ["wide_flatz", "wide_lattice"] + [f"wide_tiny{n}" for n in TINY_N] + ["wide_collapsed"]
    return f32 if wide is False else f64 if wide is True else f32 + f64


def ks_for(name):
    return K_COLLAPSED if name == "wide_collapsed" else K


def outside_queries(x, m=64):
    """m queries outside the cloud's bounds: in the shell up to half an extent
    (at least 0.5) around the box, the last quarter a full extent (at least 1)
    and more away along one axis.  Same dtype as x."""
    x = np.asarray(x)
    lo, hi = x.min(0).astype(np.float64), x.max(0).astype(np.float64)
    ext = np.maximum(hi - lo, 1.0)
    u = S.uniform_cube(m, 77).numpy().astype(np.float64)
    s = S.uniform_cube(m, 78).numpy().astype(np.float64)
    q = lo + (u * 2.0 - 0.5) * (hi - lo)
    ax = np.arange(m) % 3
    side = (np.arange(m) // 3) % 2
    far = np.where(np.arange(m) >= 3 * m // 4, 1.0 + s[:, 0], 0.05 + 0.45 * s[:, 0])
    rows = np.arange(m)
    q[rows, ax] = np.where(side == 1, hi[ax] + far * ext[ax], lo[ax] - far * ext[ax])
    return np.ascontiguousarray(q.astype(x.dtype))


def off_plane_queries(x, axis, m=32):
    """m of the cloud's points moved off its plane along `axis`, by 2^-12 to 2 on both sides."""
    x = np.asarray(x)
    q = x[:: max(1, len(x) // m)][:m].copy()
    step = 2.0 ** (np.arange(len(q)) % 14 - 12.0) * np.where(np.arange(len(q)) % 2, -1.0, 1.0)
    q[:, axis] = (q[:, axis].astype(np.float64) + step).astype(x.dtype)
    return np.ascontiguousarray(q)


# ----------------------------------------------------------------- classes
# (cloud, k) pairs whose normals are compared signed at parity.TOL: every row
# stable (stable_rows).  test_edge_clouds.test_class_table asserts that this
# table is what stable_rows gives; everything else gets the property checks.
K3 = tuple(k for k in K if k >= 3)
K8 = tuple(k for k in K if k >= 8)
SIGNED = {**{f"tiny{n}": K3 for n in TINY_N if n >= 3}, **{f"flat{a}@0": K3 for a in "xyz"},
          **{f"flat{a}@1000.5": K8 for a in "xyz"}, "line_x": K8, "lattice2d": (5, 32, 64), "flat_nested": K8}


def is_signed(name, k):
    return k in SIGNED.get(name, ())


# ------------------------------------------------------------- references
def brute_table(x, q, kmax=64, chunk=1024):
    """The kmax nearest points of every query in (d^2, index) order, by brute
    force in float64 with nanoflann's expression ((qx-x)^2+(qy-y)^2)+(qz-z)^2:
    (idx (nq, m) int32, d2 (nq, m) float64), m = min(kmax, n)."""
    x = np.asarray(x, np.float64).reshape(-1, 3)
    q = np.asarray(q, np.float64).reshape(-1, 3)
    n, nq = len(x), len(q)
    m = min(kmax, n)
    idx = np.empty((nq, m), np.int32)
    d2o = np.empty((nq, m), np.float64)
    if m == 0:
        return idx, d2o
    for a in range(0, nq, chunk):
        qq = q[a:a + chunk]
        dx = qq[:, None, 0] - x[None, :, 0]
        dy = qq[:, None, 1] - x[None, :, 1]
        dz = qq[:, None, 2] - x[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        kth = np.partition(d2, m - 1, axis=1)[:, m - 1]
        rows, cols = np.nonzero(d2 <= kth[:, None])  # every member of the k-th tie class stays in
        vals = d2[rows, cols]
        o = np.lexsort((cols, vals, rows))
        rows, cols, vals = rows[o], cols[o], vals[o]
        first = np.searchsorted(rows, np.arange(len(qq)))
        take = first[:, None] + np.arange(m)[None, :]
        idx[a:a + chunk] = cols[take]
        d2o[a:a + chunk] = vals[take]
    return idx, d2o


@functools.lru_cache(maxsize=None)
def self_table(name):
    """brute_table of the cloud `name` queried with its own points (computed once)."""
    x = cloud(name)
    return tuple(_ro(a) for a in brute_table(x, x, 64))


def brute_knn(x, q, mode, k, r=0.0, table=None):
    """KDTreeFlann search by brute force: (idx (nq, k) int32, d2 (nq, k)
    float64, count (nq,) int32) in (d^2, index) order, rows padded with -1 /
    +inf.  KNN: the k nearest; HYBRID: those of them with d^2 < r^2 (strict).
    `table`: a brute_table(x, q, kmax >= k) to cut the result from."""
    if table is None:
        table = brute_table(x, q, k)
    ti, td = table
    nq, m = ti.shape[0], min(k, ti.shape[1])
    idx = np.full((nq, k), -1, np.int32)
    d2 = np.full((nq, k), np.inf, np.float64)
    idx[:, :m] = ti[:, :m]
    d2[:, :m] = td[:, :m]
    if mode == O.HYBRID:
        out = ~(d2 < r * r)
        idx[out] = -1
        d2[out] = np.inf
    elif mode != O.KNN:
        raise ValueError("brute_knn: KNN or HYBRID")
    return idx, d2, np.sum(idx >= 0, 1).astype(np.int32)


def brute_radius(x, q1, r):
    """Every point with d^2 < r^2 of one query, in (d^2, index) order: (idx, d2)."""
    x = np.asarray(x, np.float64).reshape(-1, 3)
    q1 = np.asarray(q1, np.float64).reshape(3)
    d2 = ((q1[0] - x[:, 0]) ** 2 + (q1[1] - x[:, 1]) ** 2) + (q1[2] - x[:, 2]) ** 2
    inr = np.nonzero(d2 < r * r)[0]
    o = inr[np.lexsort((inr, d2[inr]))]
    return o.astype(np.int32), d2[o]


def radius_rows(x, r):
    """idx (n, m) / count (n,) of the RADIUS neighbourhoods of the cloud's own
    points (m = the largest count), in (d^2, index) order."""
    rows = [brute_radius(x, p, r)[0] for p in np.asarray(x, np.float64)]
    m = max(len(a) for a in rows)
    idx = np.full((len(rows), m), -1, np.int32)
    for i, a in enumerate(rows):
        idx[i, :len(a)] = a
    return idx, np.array([len(a) for a in rows], np.int32)


def raw_moments(x, idx, count):
    """Open3D ComputeCovariance's nine raw sums {x, y, z, xx, xy, xz, yy, yz,
    zz} over the first count[i] entries of row i, added one neighbour at a
    time in the row's order (float64)."""
    p = np.asarray(x, np.float64).reshape(-1, 3)
    idx = np.asarray(idx)
    count = np.asarray(count)
    m = np.zeros((len(idx), 9))
    for j in range(idx.shape[1]):
        on = j < count
        v = p[np.where(on, idx[:, j], 0)]
        t = np.stack([v[:, 0], v[:, 1], v[:, 2], v[:, 0] * v[:, 0], v[:, 0] * v[:, 1], v[:, 0] * v[:, 2],
                      v[:, 1] * v[:, 1], v[:, 1] * v[:, 2], v[:, 2] * v[:, 2]], 1)
        m = np.where(on[:, None], m + t, m)
    return m


def _normals_of(m, count):
    count = np.asarray(count)
    u = m / np.maximum(count, 1)[:, None].astype(np.float64)
    c = np.stack([u[:, 3] - u[:, 0] * u[:, 0], u[:, 4] - u[:, 0] * u[:, 1], u[:, 5] - u[:, 0] * u[:, 2],
                  u[:, 6] - u[:, 1] * u[:, 1], u[:, 7] - u[:, 1] * u[:, 2], u[:, 8] - u[:, 2] * u[:, 2]], 1)
    c[count < 3] = [1, 0, 0, 1, 0, 1]
    v = O.fast_eigen3x3(c)
    v[~np.any(v != 0, 1)] = [0.0, 0.0, 1.0]
    return v


def brute_normals(x, idx, count):
    """Open3D's normals of neighbour rows: the raw-moment covariance in the
    neighbour order, FastEigen3x3, (0,0,1) for a zero vector, the identity
    covariance below 3 neighbours."""
    return _normals_of(raw_moments(x, idx, count), count)


def stable_rows(x, idx, k, count=None, trials=8, bar=1e-6, ulps=4):
    """Rows whose normal survives another summation order: each of the nine raw
    moments is moved by up to +-ulps ulp of that moment (fixed generator),
    `trials` times; a row is stable if no normal moves more than `bar`.
    Returns (stable (n,) bool, largest move (n,))."""
    idx = np.asarray(idx)[:, :k]
    count = np.full(len(idx), idx.shape[1], np.int32) if count is None else np.minimum(np.asarray(count), k)
    m = raw_moments(x, idx, count)
    base = _normals_of(m, count)
    rng = np.random.default_rng(20240521)
    move = np.zeros(len(idx))
    for _ in range(trials):
        j = rng.integers(-ulps, ulps + 1, m.shape).astype(np.float64)
        move = np.maximum(move, np.abs(_normals_of(m + j * np.spacing(np.abs(m)), count) - base).max(1))
    return move <= bar, move


def brute_voxel(x, vs):
    """The representatives of voxel_down_sample: keys floor((p - min) / vs) in
    float64, the largest index of each voxel, ascending."""
    p = np.asarray(x, np.float64).reshape(-1, 3)
    key = np.floor((p - p.min(0)) / vs).astype(np.int64)
    last = {}
    for i, kk in enumerate(map(tuple, key)):
        last[kk] = i
    return np.array(sorted(last.values()), np.int32)


def transform_unfused(src, T):
    """((t0 x + t1 y) + t2 z) + t3 per row in float64: the ICP kernels' transform."""
    p = np.asarray(src, np.float64)
    return np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)], 1)


def brute_corr(src, tgt, T, r):
    """ICP correspondences (source row, target row), by source row: the
    (d^2, index) minimum over the target with d^2 < r^2 of the transformed
    source point."""
    idx, _, cnt = brute_knn(tgt, transform_unfused(src, T), O.HYBRID, 1, r)
    has = cnt > 0
    return np.stack([np.nonzero(has)[0], idx[has, 0].astype(np.int64)], 1)


# ------------------------------------------------------------------ radii
def cut_radius(d2k):
    """A HYBRID radius that cuts neighbourhoods: the square root of the median
    k-th neighbour d^2 (1 when that is 0: every point the same)."""
    m = float(np.median(d2k))
    r = float(np.sqrt(m)) if m > 0 else 1.0
    while m > 0 and r * r > m:  # the rows at the median itself are cut (strict <)
        r = float(np.nextafter(r, 0.0))
    return r


def below_nearest_radius(*d2):
    """Half the smallest positive distance in the given d^2 arrays (1e-3 when there is none)."""
    pos = np.concatenate([np.asarray(a).ravel() for a in d2])
    pos = pos[(pos > 0) & np.isfinite(pos)]
    return 0.5 * float(np.sqrt(pos.min())) if len(pos) else 1e-3


def mode_cases(name):
    """HYBRID / RADIUS normals cases [(mode, k, radius)] of a signed-class
    cloud: the radius holds at least kmin reference neighbours in every row,
    kmin the smallest k at which the cloud is signed (3 or 8).  RADIUS is
    left out on flat_nested, whose patch rows hold thousands of neighbours.
    test_edge_clouds.test_mode_cases_are_stable applies stable_rows to them."""
    ks = SIGNED[name]
    kmin = min(ks)
    d2 = self_table(name)[1]
    r = 1.01 * float(np.sqrt(d2[:, kmin - 1].max()))
    out = [(O.HYBRID, 16, r), (O.HYBRID, 33, r)]
    return out if name == "flat_nested" else out + [(O.RADIUS, 0, r)]


MODE_CLOUDS = tuple(n for n in SIGNED if n != "lattice2d")


def mode_rows(name, mode, k, r):
    """Reference neighbour rows (idx, count) of a mode case, in (d^2, index) order."""
    x = cloud(name)
    if mode == O.RADIUS:
        return radius_rows(x, r)
    idx, _, cnt = brute_knn(x, x, O.HYBRID, k, r, table=self_table(name))
    return idx, cnt


# -------------------------------------------------------------- ICP cases
def icp_cases():
    """name -> (target (nt,3) float32, target normals, source (ns,3) float32,
    T (4,4), max_correspondence_distance).

    lattice_tie: lattice points moved by exactly 0.5 along x lie between two
    targets at d^2 = 0.25 each (the lower index wins), those of the last
    layer and the ones put at x = -0.5 have one candidate.  lattice_at_r: the
    same with the radius exactly 0.5, every candidate at exactly r: no match
    at all; lattice_past_r: the next float64 above 0.5, every row matches.
    flat_off: the flat target's points moved off the plane by half and by
    twice the radius.  tiny*: 1 to 3 targets and sources."""
    lat = cloud("lattice3d")
    up = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (len(lat), 1))
    half = lat[:400] + np.array([0.5, 0.0, 0.0], np.float32)
    edge = lat[lat[:, 0] == 0][:40] - np.array([0.5, 0.0, 0.0], np.float32)
    src = np.concatenate([half, edge]).astype(np.float32)
    eye = np.eye(4)
    out = {"lattice_tie": (lat, up, src, eye, 0.75), "lattice_at_r": (lat, up, src, eye, 0.5),
           "lattice_past_r": (lat, up, src, eye, float(np.nextafter(0.5, 1.0)))}
    flat = cloud("flatz@0")
    r = 0.01
    s = flat[:600].copy()
    s[:, 2] += np.where(np.arange(600) % 2 == 0, np.float32(0.5 * r), np.float32(2.0 * r))
    out["flat_off"] = (flat, np.tile(up[:1], (len(flat), 1)), s, S.rigid_transform(0.05, (0, 0, 1), (0.0005, 0, 0)), r)
    T = S.rigid_transform(0.5, (1, 2, 3), (0.01, -0.02, 0.005))
    for nt in (1, 2, 3):
        for ns in (1, 2, 3):
            out[f"tiny_t{nt}_s{ns}"] = (cloud(f"tiny{nt}"), up[:nt], _u(ns, 300 + ns), T, 2.0 if ns != 2 else 0.6)
    for ns in (1, 2, 3):
        out[f"lattice_s{ns}"] = (lat, up, src[397:397 + ns], eye, 0.75)
    return out


def voxel_cases():
    """name -> (points, voxel_size): flat clouds, coincident points, tiny
    clouds, the lattice scaled by float32(0.1) at voxel_size 0.1 (every point
    on a voxel face: the float64 floor of (p - min) / vs decides), one voxel
    larger than the cloud; float32 and float64 storage."""
    out = {n: (cloud(n), 0.05) for n in FLAT}
    out["same"] = (cloud("same"), 0.1)
    for n in TINY_N:
        out[f"tiny{n}"] = (cloud(f"tiny{n}"), 0.3)
    out["lattice_faces"] = (_ro(cloud("lattice3d") * np.float32(0.1)), 0.1)
    out["one_voxel"] = (cloud("flatz@0"), 5.0)
    for n in list(out):
        out[n + "_f64"] = (_ro(out[n][0].astype(np.float64)), out[n][1])
    out["wide_flatz"] = (cloud("wide_flatz"), 0.05)
    out["wide_lattice_faces"] = (cloud("wide_lattice"), 2.0 ** -4)
    out["wide_tiny65"] = (cloud("wide_tiny65"), 0.3)
    return out


def property_checks(name, nrm, counts=None):
    """The checks of the property class: finite unit normals, none along a
    line cloud, (0,0,1) for coincident points and below 3 neighbours."""
    nrm = np.asarray(nrm, np.float64)
    assert np.isfinite(nrm).all(), name
    assert np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max(initial=0.0) <= 1e-5, name
    if name == "line_x":
        assert np.abs(nrm[:, 0]).max() <= 1e-5
    if name == "same":
        assert np.array_equal(nrm, np.tile([0.0, 0.0, 1.0], (len(nrm), 1)))
    if counts is not None:
        few = np.asarray(counts) < 3
        assert np.array_equal(nrm[few], np.tile([0.0, 0.0, 1.0], (int(few.sum()), 1))), name


# ------------------------------------------------- the library's grid rule
def search_grid(x, occ):
    """The uniform search grid the library builds over a float32 cloud for a
    target occupancy `occ`, restated from grid_build (csrc/grid.hip): the cell
    size from the density over the box's thick dimensions, one refinement when
    the occupied cells are 2.5 times denser than asked for, float32 cell
    assignment.  Returns (h, dims (3,), cell of each point, points per cell).
    Clouds below 2^20 points that fit the cell cap (asserted)."""
    x = np.asarray(x, np.float32)
    n = len(x)
    mn, mx = x.min(0).astype(np.float64), x.max(0).astype(np.float64)
    ext = np.maximum(0.0, mx - mn)
    h = ext.max() if ext.max() > 0 else 1.0
    for _ in range(4):
        thick = ext > h * 0.5
        if not ext.max() > 0 or not thick.any():
            break
        hn = (np.prod(ext[thick]) * occ / n) ** (1.0 / thick.sum())
        if abs(hn - h) <= 1e-9 * h:
            break
        h = hn
    for step in range(2):
        d = (np.floor(ext / h) + 1).astype(np.int64)
        assert n < 2 ** 20 and d.prod() <= max(4 * n, 4096)
        c = np.floor((x - mn.astype(np.float32)) * np.float32(1.0 / h)).astype(np.int64)
        c = np.clip(c, 0, d - 1)
        lin = c[:, 0] + d[0] * (c[:, 1] + d[1] * c[:, 2])
        cnt = np.bincount(lin, minlength=int(d.prod()))
        mean = n / max(int((cnt > 0).sum()), 1)
        if step == 0 and n > 64 and mean > 2.5 * occ and h * np.sqrt(occ / mean) < 0.9 * h:
            h = h * np.sqrt(occ / mean)
            continue
        break
    return h, d, lin, cnt


def knn_occupancy(k):
    """occ_for(KNN, k) of csrc/grid.hip."""
    return max(4.0, k / 3.0)


def nested_plan(x, k):
    """nested_tiles' decision (csrc/grid.hip) for KNN normals with k
    neighbours: (points in dense cells, the least a cloud needs for a nested
    grid, points the nested grid would hold, its capacity, the dense cells'
    threshold, points per cell of every point)."""
    n = len(x)
    occ = knn_occupancy(k)
    t = int(np.ceil(4.0 * occ))
    h, d, lin, cnt = search_grid(x, occ)
    g = cnt.reshape(d[2], d[1], d[0])

    def around(m):  # any of the <= 27 cells around a cell
        pad = np.pad(m, 1)
        out = np.zeros_like(m)
        for dz in range(3):
            for dy in range(3):
                for dx in range(3):
                    out |= pad[dz:dz + m.shape[0], dy:dy + m.shape[1], dx:dx + m.shape[2]]
        return out

    d1 = around(g >= t)
    d2 = (g > 0) & around(d1)
    return int(g[g >= t].sum()), max(4096, n // 32), int(g[d2].sum()), n // 2 + 4096, t, cnt[lin]
