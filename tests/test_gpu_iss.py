"""ISS keypoints, the uncapped radius count and remove_radius_outlier on the GPU
against tests/iss_oracle.py (fixtures: tests/golden/make_iss_golden.py)."""
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import iss_oracle as O  # noqa: E402
import make_iss_golden as G  # noqa: E402

pytestmark = pytest.mark.gpu

S_TOL = 1e-10  # |s - s_ref| <= S_TOL * e1_ref


@pytest.fixture(scope="module")
def clouds():
    return G.load_clouds()


def _dev_points(dev, P):
    return torch.as_tensor(np.ascontiguousarray(P), device=dev)


def _gpu_iss(dev, P, sr, nr, g21, g32, mn):
    """-> (s, count at sr, count at nr, keypoints) as numpy, through ops"""
    from open3dpypro import ops

    x = _dev_points(dev, P)
    s, cnt = ops.iss_saliency(x, sr, g21, g32, mn)
    idx = ops.iss_nms(x, s, nr, mn)
    cn = ops.radius_count(x, nr)
    assert s.dtype == torch.float64 and cnt.dtype == torch.int32 and idx.dtype == torch.int32
    return s.cpu().numpy(), cnt.cpu().numpy(), cn.cpu().numpy(), idx.cpu().numpy().astype(np.int64)


def _check_indices(s, cn, kp, mn):
    """what holds for every returned index whatever the rounding"""
    assert np.array_equal(kp, np.unique(kp))  # ascending, no repeats
    assert (s[kp] > 0).all() and (cn[kp] >= mn).all()


def _compare(got, ref, mn, what="", degenerate=False):
    """degenerate: a cloud of coplanar and collinear neighbourhoods (double
    eigenvalues at 0: e3 is rounding noise, and so are the verdicts built on
    it): the counts and the rules of the returned indices only."""
    s, cnt, cn, kp = got
    con = ref["contested"]
    assert np.array_equal(cnt, ref["count"]), what
    assert np.array_equal(cn, ref["count_nms"]), what
    _check_indices(s, cn, kp, mn)
    if degenerate:
        return
    same = (s != 0) == (ref["s"] != 0)
    assert same[~con].all(), what  # the zero / non-zero pattern outside the contested points
    err = np.abs(s - ref["s"])[same]
    bound = S_TOL * ref["e1"].astype(np.float64)[same]
    print(f"{what}: n={len(s)} keypoints={len(kp)} contested={int(con.sum())} "
          f"max |s-s_ref|/e1 = {np.max(err / np.maximum(bound / S_TOL, 1e-300), initial=0.0):.3e}")
    assert (err <= bound).all(), what
    a = np.zeros(len(s), bool)
    a[kp] = True
    b = np.zeros(len(s), bool)
    b[ref["keypoints"]] = True
    assert np.array_equal(a[~con], b[~con]), what  # the keypoint set outside the contested points


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_fixture_case(dev, clouds, name):
    from open3dpypro import ops

    cloud, params = G.CASES[name]
    P = clouds[cloud]
    assert P.dtype == (np.float64 if cloud == "wide" else np.float32)
    ref = G.load_case(name)
    sr, nr, g21, g32, mn = params
    mn = int(mn)
    x = _dev_points(dev, P)
    if sr == 0.0:
        res = ops.model_resolution(x)
        want = float(ref["radii"][2])
        print(f"{name}: resolution {res!r} oracle {want!r}")
        assert abs(res - want) <= 1e-12 * want
        assert res == ops.model_resolution(x)  # a fixed summation order
        sr, nr = 6.0 * res, 4.0 * res
        if (sr, nr) != (float(ref["radii"][0]), float(ref["radii"][1])):
            # the oracle at the radii the implementation uses: an ulp of radius decides nothing here
            ref = G.run_case(P, (sr, nr, g21, g32, mn))
        idx, sr2, nr2 = ops.iss_keypoints(x, 0.0, 0.0, g21, g32, mn)
        assert (sr2, nr2) == (sr, nr)
    else:
        idx, sr2, nr2 = ops.iss_keypoints(x, sr, nr, g21, g32, mn)
        assert (sr2, nr2) == (sr, nr)
    got = _gpu_iss(dev, P, sr, nr, g21, g32, mn)
    assert np.array_equal(idx.cpu().numpy(), got[3])  # the one-call form is the three passes
    # wide32: y keeps four values and x a few dozen: neighbourhoods in a plane or on a line
    _compare(got, ref, mn, name, degenerate=(name == "wide32_auto"))


def test_same_set_rule(dev, clouds):
    from open3dpypro import ops

    # a point and its copy have the same neighbours: the same bits, and they tie
    sr, nr, g21, g32, mn = G.CASES["dups_r"][1]
    s, _, _, kp = _gpu_iss(dev, clouds["dups"], sr, nr, g21, g32, int(mn))
    assert np.array_equal(s[0::2], s[1::2]) and (s > 0).any()
    assert len(kp) and len(kp) % 2 == 0 and (kp[0::2] % 2 == 0).all() and np.array_equal(kp[0::2] + 1, kp[1::2])
    # distinct points with the same neighbour set
    sr, nr, g21, g32, mn = G.CASES["sphere_r"][1]
    P = clouds["sphere"]
    ptr, ind = O.neighbors(P, sr)
    pairs = O.same_set_pairs(ptr, ind)
    assert len(pairs) > 0
    s, _ = ops.iss_saliency(_dev_points(dev, P), sr, g21, g32, int(mn))
    s = s.cpu().numpy()
    print(f"sphere: {len(pairs)} pairs of points with equal neighbour sets")
    assert np.array_equal(s[pairs[:, 0]], s[pairs[:, 1]])


def test_wide_cloud_through_pointcloud(dev, clouds):
    from open3dpypro import PointCloud

    P = clouds["wide"]
    pc = PointCloud(P, intensity=np.arange(len(P), dtype=np.float64).reshape(-1, 1))
    assert pc._wide
    ref = G.load_case("wide_auto")
    assert not ref["contested"].any()
    idx = pc.get_index_by_iss_keypoints()
    assert idx.dtype == np.int64 and np.array_equal(idx, ref["keypoints"])
    kc = pc.compute_iss_keypoints()
    assert kc._wide and np.array_equal(kc.get_points(), P[idx]) and np.array_equal(np.asarray(kc.intensity).reshape(-1), idx)
    # narrowed to float32 it is another cloud (a coarse lattice) with other keypoints
    narrow = PointCloud(clouds["wide32"])
    assert not narrow._wide
    nidx = narrow.get_index_by_iss_keypoints()
    assert not np.array_equal(nidx, idx)  # (its own fixture column: test_fixture_case[wide32_auto])


# ------------------------------------------------------------------ edges
def _oracle_case(P, sr, nr, g21, g32, mn):
    return G.run_case(np.asarray(P), (sr, nr, g21, g32, mn))


def _clusters(sizes, seed=5):
    """tight clusters (0.01 wide) a unit apart: at radius 0.05 each lies in a cell or two"""
    rng = np.random.default_rng(seed)
    parts = []
    for k, m in enumerate(sizes):
        c = np.array([k % 3, (k // 3) % 3, k // 9], np.float64) + 0.5
        parts.append(c + 0.01 * rng.random((m, 3)))
    P = np.concatenate(parts).astype(np.float32)
    return P[rng.permutation(len(P))]


@pytest.mark.parametrize("n", [1, 2])
def test_tiny_clouds(dev, n):
    P = np.array([[0.1, 0.2, 0.3], [0.2, 0.2, 0.3]], np.float32)[:n]
    for mn in (1, 2):
        got = _gpu_iss(dev, P, 0.5, 0.5, 0.975, 0.975, mn)
        ref = _oracle_case(P, 0.5, 0.5, 0.975, 0.975, mn)
        assert np.array_equal(got[1], np.full(n, n))
        _compare(got, ref, mn, f"n={n} min_neighbors={mn}")
    from open3dpypro import PointCloud

    assert len(PointCloud(P).get_index_by_iss_keypoints()) == 0  # automatic radii on a tiny cloud


def test_cells_around_the_tile_sizes(dev):
    """cells of 1, 7, 8, 9 queries (the staging threshold) and of 63, 64, 65
    and 129 candidates (an LDS chunk, one more, two and one more)"""
    P = _clusters([1, 7, 8, 9, 63, 64, 65, 129])
    got = _gpu_iss(dev, P, 0.05, 0.04, 0.975, 0.975, 5)
    ref = _oracle_case(P, 0.05, 0.04, 0.975, 0.975, 5)
    assert sorted(set(ref["count"].tolist())) == [1, 7, 8, 9, 63, 64, 65, 129]
    assert ref["contested"].sum() == 0
    _compare(got, ref, 5, "clusters")


@pytest.mark.parametrize("m", [63, 64, 65])
def test_one_cell_grid(dev, m):
    """radius >= the cloud's extent: a grid of one cell, every point everyone's neighbour"""
    P = np.random.default_rng(m).random((m, 3)).astype(np.float32)
    got = _gpu_iss(dev, P, 2.0, 2.0, 0.975, 0.975, 5)
    ref = _oracle_case(P, 2.0, 2.0, 0.975, 0.975, 5)
    assert (got[1] == m).all()
    # one neighbour set: one saliency, bit-equal on every point (and so every point, or none, a keypoint)
    assert (got[0] == got[0][0]).all() and len(got[3]) in (0, m)
    _compare(got, ref, 5, f"one cell, {m} points")


def test_radius_below_every_distance(dev, clouds):
    P = clouds["cube"][:500]
    got = _gpu_iss(dev, P, 1e-6, 1e-6, 0.975, 0.975, 5)
    assert (got[1] == 1).all() and (got[2] == 1).all() and (got[0] == 0).all() and len(got[3]) == 0


def _rules_only(dev, P, sr, nr, mn):
    """degenerate clouds (nearly every point contested): counts, run-to-run
    bit identity, and the rules every returned index obeys"""
    a = _gpu_iss(dev, P, sr, nr, 0.975, 0.975, mn)
    b = _gpu_iss(dev, P, sr, nr, 0.975, 0.975, mn)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    P64 = np.asarray(P, np.float64)
    assert np.array_equal(a[1], O.counts(O.neighbors_brute(P64, sr)[0]))
    assert np.array_equal(a[2], O.counts(O.neighbors_brute(P64, nr)[0]))
    _check_indices(a[0], a[2], a[3], mn)
    return a


def test_lattice_excludes_pairs_at_the_radius(dev):
    g = (np.stack(np.meshgrid(*[np.arange(9)] * 3, indexing="ij"), -1).reshape(-1, 3) * 0.125).astype(np.float32)
    a = _rules_only(dev, g, 0.25, 0.25, 5)
    centre = int(np.nonzero((g == 0.5).all(1))[0][0])
    assert a[1][centre] == 27  # 33 lattice points within 0.25 inclusive: the six at exactly 0.25 are out
    d2 = O._d2(g[centre].astype(np.float64), g.astype(np.float64))
    assert (d2 == 0.0625).sum() == 6 and (d2 <= 0.0625).sum() == 33


def test_collinear_and_coplanar(dev):
    rng = np.random.default_rng(11)
    t = np.sort(rng.random(300)).astype(np.float32)
    line = np.stack([t, 2 * t, -t], 1).astype(np.float32)
    _rules_only(dev, line, 0.1, 0.08, 3)
    plane = np.concatenate([rng.random((600, 2)), np.zeros((600, 1))], 1).astype(np.float32)
    _rules_only(dev, plane, 0.1, 0.08, 5)


def test_min_neighbors_at_the_count(dev, clouds):
    from open3dpypro import ops

    P = clouds["cube"]
    sr, nr, g21, g32, _ = G.CASES["cube_r"][1]
    ref = G.load_case("cube_r")
    i = int(np.nonzero((ref["s"] > 0) & (ref["count"] <= 12))[0][0])
    k = int(ref["count"][i])
    x = _dev_points(dev, P)
    s_at, cnt = ops.iss_saliency(x, sr, g21, g32, k)
    s_over, _ = ops.iss_saliency(x, sr, g21, g32, k + 1)
    assert int(cnt[i]) == k
    assert float(s_at[i]) > 0 and float(s_over[i]) == 0.0
    for mn in (k, k + 1):
        _compare(_gpu_iss(dev, P, sr, nr, g21, g32, mn), _oracle_case(P, sr, nr, g21, g32, mn), mn,
                 f"cube min_neighbors={mn}")


# ------------------------------------------------------- remove_radius_outlier
@pytest.mark.parametrize("nb,radius", [(5, 0.12), (1, 0.03), (40, 0.2)])
def test_remove_radius_outlier(dev, clouds, nb, radius):
    from open3dpypro import PointCloud, ops

    P = clouds["cube"]
    n = len(P)
    want = O.counts(O.neighbors(P, radius)[0])
    cnt = ops.radius_count(_dev_points(dev, P), radius).cpu().numpy()
    assert np.array_equal(cnt, want)
    capped = ops.radius_count(_dev_points(dev, P), radius, cap=nb + 1).cpu().numpy()
    assert np.array_equal(capped, np.minimum(want, nb + 1))
    keep = np.nonzero(want > nb)[0]
    assert 0 < len(keep) < n
    rgb = np.random.default_rng(1).random((n, 3))
    nrm = np.random.default_rng(2).random((n, 3)).astype(np.float32)
    pc = PointCloud(P, rgb=rgb, normals=nrm, intensity=np.arange(n, dtype=np.float64).reshape(-1, 1),
                    labels=(np.arange(n) % 7).reshape(-1, 1))
    out, kept = pc.remove_radius_outlier(nb, radius)
    assert kept == keep.tolist()
    assert np.array_equal(out.get_points().astype(np.float32), P[keep])
    assert np.array_equal(out.get_normals().astype(np.float32), nrm[keep])
    assert np.array_equal(out.get_colors(), pc.get_colors()[keep])
    assert np.array_equal(np.asarray(out.intensity).reshape(-1), keep)
    assert np.array_equal(np.asarray(out.labels).reshape(-1), keep % 7)


# ------------------------------------------------------------ the two forms
@pytest.mark.parametrize("which", ["bunny", "clusters", "wide"])
def test_tile_form_equals_lane_form(dev, clouds, monkeypatch, which):
    if which == "bunny":
        P, (sr, nr, g21, g32, mn) = clouds["bunny"], G.CASES["bunny_big"][1]
    elif which == "wide":
        P, (_, _, g21, g32, mn) = clouds["wide"], G.CASES["wide_auto"][1]
        sr, nr = (float(v) for v in G.load_case("wide_auto")["radii"][:2])
    else:
        P, (sr, nr, g21, g32, mn) = _clusters([1, 7, 8, 9, 63, 64, 65, 129]), (0.05, 0.04, 0.975, 0.975, 5)
    out = {}
    for form in ("tile", "lane"):
        monkeypatch.setenv("O3DX_ISS_FORM", form)
        out[form] = _gpu_iss(dev, P, sr, nr, g21, g32, int(mn))
    for u, v in zip(out["tile"], out["lane"]):
        assert np.array_equal(u, v)
    assert len(out["tile"][3]) > 0 or which == "clusters"


# ----------------------------------------------------------------- the recipe
def test_keypoint_restricted_registration_runs(dev, bunny):
    import globalreg_cases as GC
    from open3dpypro import (CorrespondenceCheckerBasedOnDistance, KDTreeSearchParamHybrid, PointCloud,
                             RANSACConvergenceCriteria, TransformationEstimationPointToPoint)

    src, tgt, _ = GC.bunny_pair(bunny)
    kc, kf = [], []
    for pts, par in ((src, GC.BUNNY_NORMALS_SRC), (tgt, GC.BUNNY_NORMALS_TGT)):
        pc = PointCloud(pts)
        pc.estimate_normals(param=KDTreeSearchParamHybrid(*par))
        feat = pc.compute_fpfh_feature(KDTreeSearchParamHybrid(*GC.BUNNY_FPFH))
        idx = pc.get_index_by_iss_keypoints()
        assert 3 <= len(idx) < len(pts)
        kc.append(pc._select_by_idx(idx))
        kf.append(feat.select_by_index(idx))
        assert kf[-1].num() == len(idx) == kc[-1].size() and kf[-1].dimension() == 33
        assert np.array_equal(kf[-1].data, feat.data[:, idx])
        assert np.array_equal(kc[-1].get_points(), pc.compute_iss_keypoints().get_points())
    r = kc[0].registration_ransac_based_on_feature_matching(
        kc[1], kf[0], kf[1], True, 4 * GC.BUNNY_MAX_DIST, TransformationEstimationPointToPoint(False), 3,
        [CorrespondenceCheckerBasedOnDistance(4 * GC.BUNNY_MAX_DIST)], RANSACConvergenceCriteria(10000, 0.999),
        seed=GC.BUNNY_SEED)
    T = np.asarray(r.transformation)
    assert T.shape == (4, 4) and np.isfinite(T).all() and np.isfinite(r.fitness)
