"""The neighbour search and everything on it (normals, voxel, ICP
correspondences, statistical outliers) on degenerate and tiny clouds and at
the k of the template buckets: flat, line and one-point clouds (search grids
one cell thick), integer lattices (exact distance ties at the k-th
neighbour), points at exactly the search radius (d^2 < r^2 is strict),
float64 clouds the float32 search frame collapses, 0 to 257 points.

The clouds and the plain numpy references are tests/edge_clouds.py;
test_edge_clouds.py shows on the CPU that the references equal the oracle and
which (cloud, k) pairs may be compared signed.  Every comparison here is
array_equal or parity.assert_normals (1e-5, every row).
"""
import functools

import numpy as np
import pytest
import torch

import edge_clouds as E
import open3dpypro as o3p
from oracle import oracle as O
from oracle import np_restate as NPR
from open3dpypro import ops
from parity import DebugNeighbors, assert_neighbour_sets, assert_normals

pytestmark = pytest.mark.gpu

UP = np.array([0.0, 0.0, 1.0])
LATTICE_STEP = {"lattice3d": 1.0, "lattice2d": 1.0, "wide_lattice": 2.0 ** -4}
FLAT_AXIS = {**{f"flat{a}@{c}": i for i, a in enumerate("xyz") for c in ("0", "1000.5")}, "flat_nested": 2,
             "wide_flatz": 2}
F32_ENVS = [{}, {"O3DX_NORMALS_NO_TILES": "1"}, {"O3DX_NORMALS_TOPK": "1"}, {"O3DX_NESTED_OFF": "1"}]
F64_ENVS = [{"O3DX_F64_NO_TILES": "1"}, {"O3DX_F64_NO_WAVE": "1"}, {"O3DX_F64_WAVE_KEEP": "1"}]
NORMALS_CASES = [(n, e) for n in E.names() for e in F32_ENVS + (F64_ENVS if n.startswith("wide_") else [])]


def _env_id(e):
    return "+".join(f"{k[5:]}={v}" for k, v in e.items()) or "default"


def _t(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)  # a copy: the catalogue's arrays are read-only


def _np(*ts):
    return tuple(t.cpu().numpy() for t in ts)


def _query_sets(name):
    """(what, queries, brute_table) of a cloud: its own points, 64 queries
    outside its bounds, and for a flat cloud 32 queries off its plane."""
    x = E.cloud(name)
    out = [("self", x, E.self_table(name))]
    extra = [("outside", E.outside_queries(x))]
    if name in FLAT_AXIS:
        extra.append(("off_plane", E.off_plane_queries(x, FLAT_AXIS[name])))
    return out + [(w, q, E.brute_table(x, q, 64)) for w, q in extra]


@functools.lru_cache(maxsize=None)
def _oracle_normals(name, mode, k, r):
    return O.estimate_normals(E.cloud(name), mode, k, r)


def _equal(got, ref, what):
    for g, r, part in zip(got, ref, ("idx", "d2", "count")):
        assert np.array_equal(g, r), (what, part, np.nonzero(np.any(np.atleast_2d(g.T != r.T), 0))[0][:8].tolist())


# ------------------------------------------------------------- knn_search
@pytest.mark.parametrize("name", E.names())
def test_knn_search(dev, name):
    """ops.knn_search == brute_knn (idx, d^2, count, the -1 / +inf padding of
    n < k included) for every k of the sweep: KNN; HYBRID at a radius that
    cuts the neighbourhoods, at one below the nearest neighbour (count 1 for
    the cloud's own points, 0 outside) and, on the lattices, at exactly the
    lattice step (the neighbours one step away are out) and at the next
    float64 (they are in)."""
    x = E.cloud(name)
    xd = _t(x, dev)
    sets = _query_sets(name)
    r_below = E.below_nearest_radius(*[tab[1][:, (1 if w == "self" else 0):] for w, _, tab in sets])
    for what, q, tab in sets:
        qd = _t(q, dev)
        for k in E.ks_for(name):
            tag = (name, what, k)
            _equal(_np(*ops.knn_search(xd, qd, knn=k)), E.brute_knn(x, q, O.KNN, k, table=tab), tag)
            radii = [E.cut_radius(tab[1][:, min(k, len(x)) - 1]), r_below]
            if name in LATTICE_STEP:
                radii += [LATTICE_STEP[name], float(np.nextafter(LATTICE_STEP[name], 2.0))]
            for r in radii:
                got = _np(*ops.knn_search(xd, qd, mode=O.HYBRID, knn=k, radius=r))
                _equal(got, E.brute_knn(x, q, O.HYBRID, k, r, table=tab), tag + (r,))
            if name not in ("same",):
                got = _np(*ops.knn_search(xd, qd, mode=O.HYBRID, knn=k, radius=r_below))
                assert (got[2] == (1 if what == "self" else 0)).all(), tag
            if name in LATTICE_STEP and what == "self" and k >= 8:
                at = _np(*ops.knn_search(xd, qd, mode=O.HYBRID, knn=k, radius=LATTICE_STEP[name]))[2]
                past = _np(*ops.knn_search(xd, qd, mode=O.HYBRID, knn=k,
                                           radius=float(np.nextafter(LATTICE_STEP[name], 2.0))))[2]
                assert (at == 1).all() and past.min() >= 3 and past.max() <= 7, tag


# ------------------------------------------------------------- search_one
@pytest.mark.parametrize("name", E.names())
def test_search_one(dev, name):
    """ops.search_one in its three modes == the (d^2, index) sorted brute
    force, for knn in {1, n - 1, n, n + 7}, radii that cut, lie below the
    nearest neighbour and cover everything (and the lattice step, exact and
    next), float32 and float64 storage, for a point of the cloud, a query
    outside it and one off the plane of a flat cloud."""
    x = E.cloud(name)
    n = len(x)
    stores = [x] if x.dtype == np.float64 else [x, x.astype(np.float64)]
    queries = [x[n // 2].astype(np.float64), E.outside_queries(x)[5].astype(np.float64),
               E.outside_queries(x)[60].astype(np.float64)]
    if name in FLAT_AXIS:
        queries.append(E.off_plane_queries(x, FLAT_AXIS[name])[3].astype(np.float64))
    p = x.astype(np.float64)
    for q in queries:
        d2 = ((q[0] - p[:, 0]) ** 2 + (q[1] - p[:, 1]) ** 2) + (q[2] - p[:, 2]) ** 2
        order = np.lexsort((np.arange(n), d2))
        sd = d2[order]
        radii = [E.cut_radius(sd[: min(16, n)][-1:]), E.below_nearest_radius(sd), 2.0 * float(np.sqrt(sd[-1])) + 1.0]
        if name in LATTICE_STEP:
            radii += [LATTICE_STEP[name], float(np.nextafter(LATTICE_STEP[name], 2.0))]
        for store in stores:
            xd = _t(store, dev)

            def check(mode, knn, r, exp):
                k, idx, dd = ops.search_one(xd, q, mode=mode, knn=knn, radius=r)
                tag = (name, str(store.dtype), q.tolist(), mode, knn, r)
                assert k == len(exp), tag + (k, len(exp))
                assert np.array_equal(idx.cpu().numpy(), exp), tag
                assert np.array_equal(dd.cpu().numpy(), d2[exp]), tag

            for knn in sorted({1, n - 1, n, n + 7} - {0}):
                check(O.KNN, knn, 0.0, order[:knn])
                for r in radii:
                    head = order[:knn]
                    check(O.HYBRID, knn, r, head[d2[head] < r * r])
            for r in radii:
                check(O.RADIUS, 0, r, order[sd < r * r])


# ---------------------------------------------------------------- normals
def _check_normals(name, k, got, again, count):
    assert np.array_equal(got, again), (name, k, "two runs differ")
    E.property_checks(name, got, count)


@pytest.mark.parametrize("name,env", NORMALS_CASES, ids=[f"{n}-{_env_id(e)}" for n, e in NORMALS_CASES])
def test_normals_knn(dev, name, env, monkeypatch):
    """estimate_normals(KNN k) for every k of the sweep, through the default
    chain and each forced form: the selected neighbour sets equal the
    oracle's bit for bit on every cloud (with ties the set is still unique
    under (d^2, index)); two runs are bit-identical; finite unit normals,
    (0,0,1) below 3 neighbours and for coincident points, none along the line
    cloud; and on the signed class (edge_clouds.SIGNED) every row within 1e-5
    of the oracle, signed."""
    x = E.cloud(name)
    n = len(x)
    xd = _t(x, dev)
    for kk, vv in env.items():
        monkeypatch.setenv(kk, vv)
    for k in E.ks_for(name):
        kn = min(k, n)
        with DebugNeighbors(n, kn, dev) as dn:
            got = ops.estimate_normals(xd, knn=k).cpu().numpy()
        again = ops.estimate_normals(xd, knn=k).cpu().numpy()
        tag = f"edge_{name}_{_env_id(env)}_k{k}"
        assert_neighbour_sets(dn.ids(), x, kn, tag)
        _check_normals(name, k, got, again, np.full(n, kn))
        if E.is_signed(name, k):
            assert_normals(got, _oracle_normals(name, O.KNN, k, 0.0), x, k=k, what=tag)


@pytest.mark.parametrize("name", E.MODE_CLOUDS)
def test_normals_hybrid_radius(dev, name):
    """HYBRID and RADIUS normals on the signed class, at a radius whose
    reference neighbourhoods hold at least 3 points and are stable
    (test_edge_clouds.test_mode_cases_are_stable): every row within 1e-5 of
    the oracle."""
    x = E.cloud(name)
    xd = _t(x, dev)
    for mode, k, r in E.mode_cases(name):
        got = ops.estimate_normals(xd, mode=mode, knn=k, radius=r).cpu().numpy()
        assert_normals(got, _oracle_normals(name, mode, k, r), x, mode, k, r, what=f"edge_{name}_mode{mode}_k{k}")


@pytest.mark.parametrize("name", ["lattice3d", "wide_lattice"])
@pytest.mark.parametrize("mode", [O.HYBRID, O.RADIUS])
def test_normals_lattice_radius_is_strict(dev, name, mode):
    """At a radius of exactly the lattice step every row holds its own point
    only (d^2 < r^2 is strict): the identity covariance, (0,0,1).  At the
    next float64 the 3 to 6 neighbours one step away are in: a real
    covariance, equal to brute_normals within 1e-5 on the rows that are
    stable (the cube's symmetric rows have no unique normal), finite and of
    unit length on all."""
    x = E.cloud(name)
    xd = _t(x, dev)
    step = LATTICE_STEP[name]
    got = ops.estimate_normals(xd, mode=mode, knn=16, radius=step).cpu().numpy()
    assert np.array_equal(got, np.tile(UP, (len(x), 1)).astype(np.float32))
    past = float(np.nextafter(step, 2.0))
    got = ops.estimate_normals(xd, mode=mode, knn=16, radius=past).cpu().numpy().astype(np.float64)
    idx, cnt = E.mode_rows(name, mode, 16, past)
    assert cnt.min() == 4 and cnt.max() == 7
    E.property_checks(name, got, cnt)
    stable = E.stable_rows(x, idx, idx.shape[1], cnt)[0]
    if name == "lattice3d":
        assert stable.sum() > 500
    assert np.abs(got - E.brute_normals(x, idx, cnt))[stable].max(initial=0.0) <= 1e-5


def test_normals_prior_on_flat_cloud(dev):
    x = E.cloud("flatz@0")
    prior = np.tile(-UP, (len(x), 1))
    got = ops.estimate_normals(_t(x, dev), knn=16, prior=_t(prior.astype(np.float32), dev)).cpu().numpy()
    assert_normals(got, O.estimate_normals(x, O.KNN, 16, prior=prior), x, k=16, prior=prior, what="edge_flatz_prior")
    assert np.array_equal(got, prior.astype(np.float32))


@pytest.mark.parametrize("name,vs", [("flatz@0", 0.05), ("flat_nested", 0.02)])
def test_normals_voxel_grid_paths(dev, name, vs):
    """voxel_down_sample(keep_grid=True) + estimate_normals(voxel_grid=) and
    the one-call voxel_down_sample_normals on flat clouds: the
    representatives are the oracle's, the one-call normals equal the two-call
    ones bit for bit, the neighbour sets are the oracle's, and the normals
    are within 1e-5 of the oracle's where every row of the representatives'
    cloud is stable (edge_clouds.stable_rows), with the property checks
    otherwise."""
    x = E.cloud(name)
    xd = _t(x, dev)
    a = ops.voxel_down_sample(xd, vs, keep_grid=True)
    ref = O.voxel_down_sample(x, vs)
    assert np.array_equal(a["rep_idx"].cpu().numpy(), ref)
    reps = x[ref]
    assert np.array_equal(a["rep_xyz"].cpu().numpy(), reps)
    assert a["voxel_grid"] is not None  # a flat cloud's voxel table is kept: the table path runs
    tab = E.brute_table(reps, reps, 64)
    for k in (5, 30):
        with DebugNeighbors(len(reps), k, dev) as dn:
            two = ops.estimate_normals(a["rep_xyz"], knn=k, voxel_grid=a["voxel_grid"])
        assert_neighbour_sets(dn.ids(), reps, k, f"edge_vox_{name}_k{k}")
        f = ops.voxel_down_sample_normals(xd, vs, knn=k)
        assert torch.equal(f["rep_idx"], a["rep_idx"]) and torch.equal(f["rep_xyz"], a["rep_xyz"])
        assert torch.equal(f["normals"], two)
        got = two.cpu().numpy()
        idx, _, cnt = E.brute_knn(reps, reps, O.KNN, k, table=tab)
        E.property_checks(name, got, cnt)
        if E.stable_rows(reps, idx, k, cnt)[0].all():
            assert_normals(got, O.estimate_normals(reps, O.KNN, k), reps, k=k, what=f"edge_vox_{name}_k{k}")


# ------------------------------------------------------------------ voxel
@pytest.mark.parametrize("name", sorted(E.voxel_cases()))
def test_voxel_down_sample(dev, name):
    """Representatives, voxel of every point and the cubic ids equal the
    oracle's (and the representatives brute_voxel's) on flat clouds,
    coincident points, tiny clouds, points on voxel faces and one voxel
    larger than the cloud; float32 and float64 storage."""
    x, vs = E.voxel_cases()[name]
    xd = _t(x, dev)
    rep, vop, cub = O.voxel_down_sample(x, vs, trace=True)
    assert np.array_equal(E.brute_voxel(x, vs), rep)
    out = ops.voxel_down_sample(xd, vs)
    assert np.array_equal(out["rep_idx"].cpu().numpy(), rep)
    assert np.array_equal(out["rep_xyz"].cpu().numpy(), x[rep])
    out = ops.voxel_down_sample(xd, vs, trace=True)
    assert np.array_equal(out["rep_idx"].cpu().numpy(), rep)
    assert np.array_equal(out["voxel_of_point"].cpu().numpy(), vop)
    assert np.array_equal(out["cubic_id"].cpu().numpy(), cub)


# -------------------------------------------------------------------- ICP
def _pairs(corr):
    c = corr.cpu().numpy().astype(np.int64).reshape(-1, 2)
    return c[np.argsort(c[:, 0], kind="stable")]


@pytest.mark.parametrize("estimation", ["point_to_plane", "point_to_point"])
@pytest.mark.parametrize("name", sorted(E.icp_cases()))
def test_icp_correspondences(dev, name, estimation):
    """ICPTarget.accumulate's correspondence set == brute_corr (the (d^2,
    index) minimum with d^2 < r^2: the lower index on an exact tie, no match
    at exactly max_correspondence_distance), sums[28] the count, for the
    source in the caller's order and spatially sorted; the point-to-plane
    moments equal the oracle's."""
    tgt, tn, src, T, r = E.icp_cases()[name]
    exp = E.brute_corr(src, tgt, T, r)
    target = ops.ICPTarget(_t(tgt, dev), _t(tn, dev), r)
    sd = _t(src, dev)
    for s in (sd, ops.spatial_sort(sd)):
        sums, corr = target.accumulate(s, T, want_corr=True, estimation=estimation)
        assert np.array_equal(_pairs(corr), exp), name
        assert sums[28] == len(exp)
        q = E.transform_unfused(src, T)[exp[:, 0]]
        t = tgt.astype(np.float64)[exp[:, 1]]
        d = q - t  # sums[29]: the squared correspondence distances, whatever the estimation
        np.testing.assert_allclose(sums[29], float(((d[:, 0] ** 2 + d[:, 1] ** 2) + d[:, 2] ** 2).sum()), rtol=1e-9,
                                   atol=1e-9)
        if estimation == "point_to_plane":
            ref = O.icp_accumulate(src, tgt, tn, r, T)
            assert sums[28] == ref[28]
            np.testing.assert_allclose(sums[:30], ref[:30], rtol=1e-9, atol=1e-9)


# ---------------------------------------------------- statistical outliers
@pytest.mark.parametrize("name", ["flatz@0", "same"] + [f"tiny{n}" for n in E.TINY_N])
def test_remove_statistical_outlier(name):
    x = E.cloud(name)
    _, idx = o3p.PointCloud(x.astype(np.float64)).remove_statistical_outlier(20, 2.0)
    d2 = E.brute_knn(x, x, O.KNN, min(20, len(x)), table=E.self_table(name))[1]
    assert idx == NPR.remove_statistical_outlier(x, 20, 2.0, d2).tolist()


# ------------------------------------------------------------ empty cloud
def test_empty_cloud(dev):
    """n = 0.  o3dx_knn_search builds the grid of an empty cloud (the bounds
    kernels read nothing and write zeros, one cell, every n-sized launch
    skipped) and k_knn_query returns 0 for every query on g.n == 0 before it
    touches the grid: count 0, -1 and +inf.  search_one and estimate_normals
    return before any launch."""
    empty = torch.zeros((0, 3), dtype=torch.float32, device=dev)
    q = _t(E.cloud("tiny65"), dev)
    for mode, r in ((O.KNN, 0.0), (O.HYBRID, 0.5)):
        idx, d2, cnt = _np(*ops.knn_search(empty, q, mode=mode, knn=5, radius=r))
        assert idx.shape == (65, 5) and (idx == -1).all() and np.isposinf(d2).all() and (cnt == 0).all()
    for mode in (O.KNN, O.RADIUS, O.HYBRID):
        k, idx, d2 = ops.search_one(empty, [0.1, 0.2, 0.3], mode=mode, knn=4, radius=1.0)
        assert k == 0 and idx.numel() == 0 and d2.numel() == 0
    assert tuple(ops.estimate_normals(empty, knn=30).shape) == (0, 3)
