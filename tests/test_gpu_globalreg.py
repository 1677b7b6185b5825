"""GPU tests of FPFH, the feature matcher and RANSAC on correspondences against
the numpy restatement (tests/globalreg_oracle.py)."""
import os

import numpy as np
import pytest
import torch

import globalreg_cases as GC
import globalreg_oracle as GO
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

MODES = {"knn": 0, "hybrid": 2}


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "globalreg_ref.npz"))


@pytest.fixture(scope="module")
def pair(bunny):
    return GC.bunny_pair(bunny)


def _gpu_fpfh(dev, pts, nrm, mode, knn, radius):
    from open3dpypro import ops

    f, counts, m = ops.fpfh(torch.as_tensor(pts, device=dev), torch.as_tensor(nrm, device=dev), MODES[mode], knn,
                            radius, return_spfh=True)
    return f.cpu().numpy(), counts.cpu().numpy(), m.cpu().numpy()


def _check_fpfh(dev, pts, nrm, mode, knn, radius, diag=None):
    idx, d2, cnt = GC.lists_of(pts, mode, knn, radius)
    want, wcounts, _ = GO.fpfh(pts, nrm, idx, d2, cnt, diag)
    f, counts, m = _gpu_fpfh(dev, pts, nrm, mode, knn, radius)
    assert f.shape == (len(pts), 33) and f.dtype == np.float32
    assert np.array_equal(m.astype(np.int64), np.asarray(cnt).astype(np.int64))
    assert np.array_equal(counts.astype(np.int64), wcounts)  # the integer bin counts, exactly
    err = np.abs(f.astype(np.float64) - want).max() if len(pts) else 0.0
    print(f"fpfh n={len(pts)} max|err|={err:.3e}")
    assert err < 1e-4  # every entry of every row
    return f


@pytest.mark.parametrize("name", sorted(GC.fpfh_cases()))
def test_fpfh_small_cases(dev, name):
    pts, nrm, mode, knn, radius = GC.fpfh_cases()[name]
    diag = {}
    _check_fpfh(dev, pts, nrm, mode, knn, radius, diag)
    if diag:  # the conditions under which the integer counts compare exactly
        assert diag["bin_edge_min"] > 1e-9 and diag["acos_gap_min"] > 1e-12, diag


@pytest.fixture(scope="module")
def bunny_gpu(dev, pair):
    """Normals and features of the bunny pair through PointCloud, once."""
    from open3dpypro import KDTreeSearchParamHybrid, PointCloud

    out = []
    for pts, par in ((pair[0], GC.BUNNY_NORMALS_SRC), (pair[1], GC.BUNNY_NORMALS_TGT)):
        pc = PointCloud(pts)
        pc.estimate_normals(param=KDTreeSearchParamHybrid(*par))
        feat = pc.compute_fpfh_feature(KDTreeSearchParamHybrid(*GC.BUNNY_FPFH))
        out.append((pc, feat))
    return out


def test_fpfh_bunny_pair(dev, pair, bunny_gpu):
    for (pc, feat), pts in zip(bunny_gpu, pair[:2]):
        nrm = pc.get_normals().astype(np.float32)
        diag = {}
        f = _check_fpfh(dev, pts, nrm, "hybrid", GC.BUNNY_FPFH[1], GC.BUNNY_FPFH[0], diag)
        assert diag["bin_edge_min"] > 1e-9 and diag["acos_gap_min"] > 1e-12, diag
        assert feat.data.shape == (33, len(pts)) and feat.data.dtype == np.float64
        assert (feat.dimension(), feat.num()) == (33, len(pts))
        assert np.array_equal(feat.data.T.astype(np.float32), f)  # PointCloud's is the same call


@pytest.mark.parametrize("name", sorted(GC.match_cases()))
def test_feature_match_cases(dev, name):
    from open3dpypro import ops

    a, b = GC.match_cases()[name]
    want, gap = GO.match(a, b)
    # the comparison is exact where the float64 gap is 0 (a tie: lowest index)
    # or beyond the float32 kernel's 33 roundings
    assert not ((gap != 0.0) & ~(gap > 1e-5)).any()
    A, B = torch.as_tensor(a, device=dev), torch.as_tensor(b, device=dev)
    got = ops.feature_match(A, B).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, want)
    for mutual in (False, True):
        for ratio in (0.1, 0.99):
            c = ops.correspondences_from_features(A, B, mutual, ratio).cpu().numpy()
            w = GO.correspondences(a, b, mutual, ratio)
            assert c.dtype == np.int32 and c.shape == w.shape and np.array_equal(c, w)
    if name == "random_257x130":
        m = GO.correspondences(a, b, True, 0.1)
        assert 0 < len(m) < len(a)  # the mutual set, not the fallback
        assert len(GO.correspondences(a, b, True, 0.99)) == len(a)  # the fallback


def test_feature_match_bunny_against_fixture(dev, ref, pair, bunny_gpu):
    """On the restatement's own float32 features (every row, rebuilt on the
    CPU) the matcher gives the stored correspondences."""
    from open3dpypro import ops
    from oracle import oracle as O

    feats = []
    for pts, par in ((pair[0], GC.BUNNY_NORMALS_SRC), (pair[1], GC.BUNNY_NORMALS_TGT)):
        nrm = O.estimate_normals(pts, O.HYBRID, par[1], par[0]).astype(np.float32)
        idx, d2, cnt = O.knn_search(pts, pts, O.HYBRID, GC.BUNNY_FPFH[1], GC.BUNNY_FPFH[0])
        feats.append(GO.fpfh(pts, nrm, idx, d2, cnt)[0].astype(np.float32))
    c = ops.correspondences_from_features(torch.as_tensor(feats[0], device=dev), torch.as_tensor(feats[1], device=dev),
                                          mutual_filter=True)
    assert np.array_equal(c.cpu().numpy(), ref["corres"])


def _np_scores(src, tgt, corr, Ts, max_d):
    p = src.astype(np.float64)[corr[:, 0]]
    q = tgt.astype(np.float64)[corr[:, 1]]
    counts, sums = [], []
    for T in Ts:
        c, e2, _ = GO.score(T, p, q, max_d)
        counts.append(c)
        sums.append(e2)
    return np.int64(counts), np.float64(sums)


@pytest.mark.parametrize("C,H", [(1, 1), (63, 7), (64, 7), (65, 7), (554, 1), (554, 4096), (65, 4096)])
def test_corr_count_and_error2(dev, C, H):
    from open3dpypro import ops

    src, tgt, corr, Ts = GC.scorer_case(C, H)
    max_d = 0.05
    S, T = torch.as_tensor(src, device=dev), torch.as_tensor(tgt, device=dev)
    got = ops.corr_count(S, T, corr, Ts, max_d)
    p = src.astype(np.float64)[corr[:, 0]]
    q = tgt.astype(np.float64)[corr[:, 1]]
    want = (GO.transform_dist(Ts, p, q) < max_d).sum(1)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert want.max() > 0
    which = np.unique(np.r_[0, np.argsort(want)[-3:]])
    sums, counts = ops.corr_error2(S, T, corr, Ts[which], max_d, return_counts=True)
    wc, ws = _np_scores(src, tgt, corr, Ts[which], max_d)
    assert np.array_equal(counts, wc)
    np.testing.assert_allclose(sums, ws, rtol=1e-12, atol=0)
    # bit-identical reruns
    assert np.array_equal(ops.corr_count(S, T, corr, Ts, max_d), got)
    assert np.array_equal(ops.corr_error2(S, T, corr, Ts[which], max_d), sums)


def test_corr_count_exact_threshold(dev):
    from open3dpypro import ops

    src, tgt, corr, Ts, max_d, want = GC.exact_threshold_case()
    S, T = torch.as_tensor(src, device=dev), torch.as_tensor(tgt, device=dev)
    assert np.array_equal(ops.corr_count(S, T, corr, Ts, max_d), want)  # d == max is not an inlier, d == 0 is
    sums, counts = ops.corr_error2(S, T, corr, Ts, max_d, return_counts=True)
    assert np.array_equal(counts, want)
    np.testing.assert_allclose(sums, [4.0, 1.0 + 5.0, 0.0], rtol=1e-12, atol=0)  # (sqrt(5)^2 is not 5)
    with pytest.raises(RuntimeError, match="out of range"):
        ops.corr_count(S, T, np.int32([[0, 4]]), Ts, max_d)


def test_ransac_given_the_committed_samples(dev, ref, pair):
    from open3dpypro import ops

    src, tgt, _ = pair
    S, T = torch.as_tensor(src, device=dev), torch.as_tensor(tgt, device=dev)
    res = {}
    for rs in (64, 4096):
        res[rs] = ops.registration_ransac_based_on_correspondence(
            S, T, ref["corres"], GC.BUNNY_MAX_DIST, 3, GC.BUNNY_EDGE, GC.BUNNY_MAX_DIST, len(ref["samples"]), 0.999,
            samples=ref["samples"], round_size=rs)
    r = res[4096]
    assert r["best_iteration"] == int(ref["best_iteration"])
    assert r["processed"] == int(ref["processed"]) and r["scored"] == int(ref["scored"])
    np.testing.assert_allclose(r["transformation"], ref["T"], rtol=0, atol=1e-9)
    assert r["corr_fitness"] == int(ref["count"]) / len(ref["corres"])
    np.testing.assert_allclose(r["corr_rmse"], np.sqrt(float(ref["err2"]) / int(ref["count"])), rtol=1e-12)
    for k in r:
        assert np.array_equal(res[64][k], r[k]), k  # the round size changes nothing
    # the seeded sampler reproduces the committed list: the same call by seed
    by_seed = ops.registration_ransac_based_on_correspondence(
        S, T, ref["corres"], GC.BUNNY_MAX_DIST, 3, GC.BUNNY_EDGE, GC.BUNNY_MAX_DIST, GC.BUNNY_MAX_ITER, 0.999,
        seed=int(ref["seed"]))
    assert by_seed["best_iteration"] == r["best_iteration"] and by_seed["processed"] == r["processed"]


def test_end_to_end_through_pointcloud(dev, pair, bunny_gpu):
    from open3dpypro import (CorrespondenceCheckerBasedOnDistance, CorrespondenceCheckerBasedOnEdgeLength,
                             RANSACConvergenceCriteria, TransformationEstimationPointToPoint)

    (spc, sf), (tpc, tf) = bunny_gpu
    r = spc.registration_ransac_based_on_feature_matching(
        tpc, sf, tf, True, GC.BUNNY_MAX_DIST, TransformationEstimationPointToPoint(False), 3,
        [CorrespondenceCheckerBasedOnEdgeLength(GC.BUNNY_EDGE), CorrespondenceCheckerBasedOnDistance(GC.BUNNY_MAX_DIST)],
        RANSACConvergenceCriteria(GC.BUNNY_MAX_ITER, 0.999), seed=GC.BUNNY_SEED)
    rot, tr = GC.pose_error(r.transformation, pair[2])
    print(f"ransac: fitness {r.fitness:.3f} rmse {r.inlier_rmse:.5f} pose error {rot:.3f} deg {tr:.5f}")
    assert r.fitness > 0 and len(r.correspondence_set) == round(r.fitness * spc.size())
    # the result is the evaluation of the winning transformation over every source point
    ev = spc.evaluate_registration(tpc, GC.BUNNY_MAX_DIST, r.transformation)
    assert ev.fitness == r.fitness and ev.inlier_rmse == r.inlier_rmse
    assert np.array_equal(ev.transformation, r.transformation)
    icp = spc.registration_icp(tpc, GC.BUNNY_MAX_DIST, init=r.transformation, estimation="point_to_plane")
    rot, tr = GC.pose_error(icp.transformation, pair[2])
    print(f"icp: fitness {icp.fitness:.3f} pose error {rot:.4f} deg {tr:.6f}")
    assert rot < 0.2 and tr < 5e-4


def test_evaluate_registration_is_icp_at_zero_iterations(dev, pair):
    """registration_icp(max_iteration=0) reports the 1-NN-within-distance
    evaluation of init, against brute force."""
    from open3dpypro import PointCloud

    src, tgt, T = pair
    s, t = PointCloud(src[:400]), PointCloud(tgt)
    r = s.evaluate_registration(t, 0.004, T)
    assert np.array_equal(r.transformation, T)
    p = src[:400].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    d2 = ((p[:, None, :] - tgt.astype(np.float64)[None]) ** 2).sum(2)
    j = d2.argmin(1)
    inl = d2[np.arange(len(p)), j] < 0.004 ** 2
    assert 0 < inl.sum() < len(p)
    assert r.fitness == inl.sum() / len(p)
    np.testing.assert_allclose(r.inlier_rmse, np.sqrt(d2[np.arange(len(p)), j][inl].mean()), rtol=1e-9)
    assert np.array_equal(r.correspondence_set[:, 0], np.nonzero(inl)[0])


def test_bit_identical_reruns(dev, pair, bunny_gpu):
    from open3dpypro import ops

    pc, feat = bunny_gpu[1]
    a = ops.fpfh(pc._dev_points(), pc._normals, 2, GC.BUNNY_FPFH[1], GC.BUNNY_FPFH[0])
    b = ops.fpfh(pc._dev_points(), pc._normals, 2, GC.BUNNY_FPFH[1], GC.BUNNY_FPFH[0])
    assert torch.equal(a, b) and torch.equal(a, feat.device_rows())
    fs, ft = bunny_gpu[0][1].device_rows(), feat.device_rows()
    i1, d1 = ops.feature_match(fs, ft, return_d2=True)
    i2, d2 = ops.feature_match(fs, ft, return_d2=True)
    assert torch.equal(i1, i2) and torch.equal(d1, d2)


def test_bad_arguments(dev):
    from open3dpypro import (KDTreeSearchParamHybrid, KDTreeSearchParamRadius, PointCloud,
                             TransformationEstimationPointToPlane, ops)

    rng = np.random.default_rng(0)
    p = rng.uniform(0, 1, (50, 3)).astype(np.float32)
    nrm = np.tile(np.float32([0, 0, 1]), (50, 1))
    pc = PointCloud(p, normals=nrm)
    with pytest.raises(ValueError, match="64"):
        pc.compute_fpfh_feature(KDTreeSearchParamHybrid(0.5, 65))
    with pytest.raises(NotImplementedError):
        pc.compute_fpfh_feature(KDTreeSearchParamRadius(0.5))
    with pytest.raises(RuntimeError, match="normal"):
        PointCloud(p).compute_fpfh_feature(KDTreeSearchParamHybrid(0.5, 30))
    wide = PointCloud(np.float64([[1e9 + 0.125, 0, 0], [1e9 + 0.25, 1, 0], [1e9 + 0.375, 0, 1]]),
                      normals=nrm[:3])
    with pytest.raises(NotImplementedError, match="float64"):
        wide.compute_fpfh_feature(KDTreeSearchParamHybrid(0.5, 30))
    f = pc.compute_fpfh_feature(KDTreeSearchParamHybrid(0.5, 30))
    with pytest.raises(ValueError):
        pc.registration_ransac_based_on_feature_matching(pc, f, f, False, 0.1, TransformationEstimationPointToPlane())
    x = torch.as_tensor(p, device=dev)
    with pytest.raises(ValueError, match="64"):
        ops.fpfh(x, torch.as_tensor(nrm, device=dev), 0, 65)
    with pytest.raises(NotImplementedError):
        ops.fpfh(x, torch.as_tensor(nrm, device=dev), 1, 10, 0.5)
    with pytest.raises(RuntimeError):
        ops.feature_match(torch.zeros((4, 32), device=dev), torch.zeros((4, 33), device=dev))
