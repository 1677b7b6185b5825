"""CPU tests of the global-registration layer: the numpy restatement
(tests/globalreg_oracle.py) against the stored fixture, its invariants, the
host helpers of libo3dx (batched Umeyama, checkers) and the Python layer's
selection replay, errors and empty results.  No GPU."""
import os

import numpy as np
import pytest

import globalreg_cases as GC
import globalreg_oracle as GO
from conftest import GOLDEN


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "globalreg_ref.npz"))


@pytest.fixture(scope="module")
def pair(bunny):
    return GC.bunny_pair(bunny)


@pytest.fixture(scope="module")
def bunny_feats(pair):
    """The restatement's float32 features of the bunny pair, once."""
    from oracle import oracle as O

    out = []
    for pts, par in ((pair[0], GC.BUNNY_NORMALS_SRC), (pair[1], GC.BUNNY_NORMALS_TGT)):
        nrm = O.estimate_normals(pts, O.HYBRID, par[1], par[0]).astype(np.float32)
        idx, d2, cnt = O.knn_search(pts, pts, O.HYBRID, GC.BUNNY_FPFH[1], GC.BUNNY_FPFH[0])
        out.append(GO.fpfh(pts, nrm, idx, d2, cnt)[0].astype(np.float32))
    return out


def test_restatement_features_match_fixture(ref, pair, bunny_feats):
    assert [len(pair[0]), len(pair[1])] == ref["sizes"].tolist()
    step = int(ref["row_step"])
    # the stored rows were computed by the same code; libm may differ by an ulp
    # of float64 between machines, far below a float32 ulp of 200
    np.testing.assert_allclose(bunny_feats[0][::step], ref["feat_src"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(bunny_feats[1][::step], ref["feat_tgt"], rtol=0, atol=1e-4)


def test_restatement_correspondences_and_ransac_match_fixture(ref, pair, bunny_feats):
    corres = GO.correspondences(bunny_feats[0], bunny_feats[1], mutual_filter=True)
    assert np.array_equal(corres, ref["corres"])
    r = GO.ransac(pair[0], pair[1], ref["corres"], ref["samples"], GC.BUNNY_MAX_DIST, 3, GC.BUNNY_EDGE,
                  GC.BUNNY_MAX_DIST, 0.999)
    # the stored head of the sample list ends after the rule's stop
    assert r["processed"] == int(ref["processed"]) < len(ref["samples"])
    assert r["best_iteration"] == int(ref["best_iteration"])
    assert r["scored"] == int(ref["scored"]) and r["count"] == int(ref["count"])
    np.testing.assert_allclose(r["T"], ref["T"], rtol=0, atol=1e-9)
    rot, tr = GC.pose_error(r["T"], pair[2])
    assert rot < 5.0 and tr < 0.01


def test_fixture_samples_are_the_librarys(ref):
    from open3dpypro import ops

    s = ops.ransac_samples(len(ref["corres"]), 3, len(ref["samples"]), int(ref["seed"]))
    assert np.array_equal(s, ref["samples"])


@pytest.mark.parametrize("name", sorted(GC.fpfh_cases()))
def test_fpfh_invariants(name):
    pts, nrm, mode, knn, radius = GC.fpfh_cases()[name]
    idx, d2, cnt = GC.lists_of(pts, mode, knn, radius)
    f, counts, spfh = GO.fpfh(pts, nrm, idx, d2, cnt)
    assert f.shape == (len(pts), 33)
    m = np.asarray(cnt).astype(np.int64)
    assert (f[m <= 1] == 0).all()
    # every list position but the first votes once per group
    assert np.array_equal(counts.reshape(len(pts), 3, 11).sum(2), np.repeat(np.maximum(m - 1, 0)[:, None], 3, 1))
    live = m > 1
    np.testing.assert_allclose(spfh[live].sum(1), 300.0, rtol=1e-9)
    g = f.reshape(len(pts), 3, 11).sum(2)
    # the SPFH row's 100 plus the second pass's normalised 100 (only 100 where
    # every listed neighbour is a duplicate of the point)
    some = live & ((np.arange(idx.shape[1])[None, :] >= 1) & (np.arange(idx.shape[1])[None, :] < m[:, None])
                   & (d2 != 0)).any(1) if len(pts) else live
    np.testing.assert_allclose(g[some], 200.0, rtol=1e-9)
    np.testing.assert_allclose(g[live & ~some], 100.0, rtol=1e-9)


def test_fpfh_case_coverage():
    """The cases hit what they are there for."""
    cases = GC.fpfh_cases()
    pts, nrm, mode, knn, radius = cases["bumpy_hybrid"]
    cnt = GC.lists_of(pts, mode, knn, radius)[2]
    assert cnt.min() < cnt.max() and cnt.max() == knn
    pts, nrm, mode, knn, radius = cases["isolated_hybrid"]
    assert (GC.lists_of(pts, mode, knn, radius)[2] == 1).sum() == 7
    pts, nrm, mode, knn, radius = cases["duplicates"]
    assert (GC.lists_of(pts, mode, knn, radius)[1][:, 1] == 0).sum() >= 80
    # the stacked column: dp parallel to the shared normal gives the zero feature
    pts, nrm, mode, knn, radius = cases["lattice_column"]
    f0, f1, f2 = GO.pair_features(pts[-1:].astype(np.float64), nrm[-1:].astype(np.float64),
                                  pts[-2:-1].astype(np.float64), nrm[-2:-1].astype(np.float64))
    assert f0[0] == 0 and f1[0] == 0 and f2[0] == 0


def test_pair_feature_acos_rule_is_not_abs_compare():
    """Near 0 acos is flat: different |a| give equal acos values, and the rule
    compares the acos values."""
    a1, a2 = 1e-17, 3e-17
    assert np.arccos(a1) == np.arccos(a2) and a1 < a2


def test_match_restatement_lowest_index_on_ties():
    a, b = GC.match_cases()["duplicates_257x130"]
    idx, gap = GO.match(a, b)
    assert (idx[:16] == np.arange(5, 21)).all() and (gap[:16] == 0).all()
    c = GO.correspondences(a, b, mutual_filter=True)
    assert (np.diff(c[:, 0]) > 0).all()


def _samples_case(C, iters, seed):
    src, tgt, corr, _ = GC.scorer_case(C, 1, seed)
    rng = np.random.default_rng(seed)
    smp = np.stack([rng.permutation(C)[:3] for _ in range(iters)]).astype(np.int32)
    return src, tgt, corr, smp


def test_batched_umeyama_against_numpy_svd():
    from open3dpypro import ops

    src, tgt, corr, smp = _samples_case(65, 500, 3)
    p = src.astype(np.float64)[corr[:, 0]][smp]
    q = tgt.astype(np.float64)[corr[:, 1]][smp]
    T = ops.umeyama_from_samples(np.stack([p, q], axis=2))
    np.testing.assert_allclose(T, GO.umeyama(p, q), rtol=0, atol=1e-12)
    # a rank-deficient sample (three times the same pair): the identity
    one = np.stack([np.repeat(p[:1, :1], 3, 1), np.repeat(q[:1, :1], 3, 1)], axis=2)
    assert np.array_equal(ops.umeyama_from_samples(one)[0], np.eye(4))


def test_host_checkers_against_restatement():
    from open3dpypro import ops

    src, tgt, corr, smp = _samples_case(65, 800, 4)
    p = src.astype(np.float64)[corr[:, 0]][smp]
    q = tgt.astype(np.float64)[corr[:, 1]][smp]
    coords = np.stack([p, q], axis=2)
    T = GO.umeyama(p, q)
    e = GO.check_edge_length(p, q, 0.9)
    d = GO.check_distance(p, q, T, 0.03)
    assert 0 < e.sum() < len(e) and 0 < d.sum() < len(d)
    assert np.array_equal(ops.corr_check(coords, T, 0.9, -1.0), e)
    assert np.array_equal(ops.corr_check(coords, T, -1.0, 0.03), d)
    assert np.array_equal(ops.corr_check(coords, T, 0.9, 0.03), e & d)
    assert ops.corr_check(coords, T).all()


@pytest.mark.parametrize("C,iters,max_d,round_size", [(20, 400, 0.03, 7), (20, 400, 0.03, 4096), (65, 3000, 0.04, 64),
                                                      (12, 300, 0.05, 1), (65, 50, 1e-9, 16)])
def test_selection_replay_against_restatement(C, iters, max_d, round_size):
    """The round driver with numpy scorers in place of the GPU sweeps picks
    the restatement's winner and stops where it stops, whatever the round size
    (small C: many fitness ties)."""
    from open3dpypro import ops

    src, tgt, corr, smp = _samples_case(C, iters, 5)
    p = src.astype(np.float64)[corr[:, 0]]
    q = tgt.astype(np.float64)[corr[:, 1]]
    calls = {"err2": 0}

    def count_fn(T):
        return np.array([GO.score(t, p, q, max_d)[0] for t in T], np.int64)

    def err2_fn(T):
        calls["err2"] += len(T)
        return np.array([GO.score(t, p, q, max_d)[1] for t in T])

    got = ops.corr_ransac_rounds(p, q, smp, 3, 0.9, -1.0, iters, 0.999, round_size, count_fn, err2_fn)
    T_all = ops.umeyama_from_samples(np.stack([p[smp], q[smp]], axis=2))
    want = GO.ransac(src, tgt, corr, smp, max_d, 3, 0.9, None, 0.999, transforms=T_all)
    assert got["best_iteration"] == want["best_iteration"]
    assert got["processed"] == want["processed"] and got["scored"] == want["scored"]
    np.testing.assert_array_equal(got["transformation"], want["T"])
    if want["count"]:
        assert got["corr_fitness"] == want["count"] / C
        np.testing.assert_allclose(got["corr_rmse"], np.sqrt(want["err2"] / want["count"]), rtol=1e-12)
    else:
        assert got["best_iteration"] == -1 and got["corr_fitness"] == 0.0
    assert calls["err2"] <= 2 * want["scored"] + 1


def test_est_k_rule():
    from open3dpypro import ops

    assert ops.ransac_est_k(1.0, 3, 0.999) == 0.0
    assert ops.ransac_est_k(1e-9, 3, 0.999) == np.inf
    assert ops.ransac_est_k(0.5, 3, 0.999) == pytest.approx(np.log(0.001) / np.log(1 - 0.125), rel=1e-15)


# ------------------------------------------------------- the Python layer
def _cloud(n=10, normals=False):
    from open3dpypro import PointCloud

    rng = np.random.default_rng(n)
    p = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    return PointCloud(p, normals=np.tile(np.float32([0, 0, 1]), (n, 1)) if normals else None)


def test_param_classes_are_duck_typed():
    from open3dpypro import params as P

    c = P.RANSACConvergenceCriteria()
    assert (c.max_iteration, c.confidence) == (100000, 0.999)

    class Edge:
        similarity_threshold = 0.8

    class Dist:
        distance_threshold = 0.5

    class Normal:
        normal_angle_threshold = 0.1

    assert P.resolve_checkers([Edge(), Dist()]) == (0.8, 0.5)
    assert P.resolve_checkers([]) == (-1.0, -1.0)
    assert P.resolve_checkers([P.CorrespondenceCheckerBasedOnEdgeLength(0.9),
                               P.CorrespondenceCheckerBasedOnDistance(0.1)]) == (0.9, 0.1)
    with pytest.raises(ValueError):
        P.resolve_checkers([Normal()])
    with pytest.raises(ValueError):
        P.resolve_checkers([object()])


def test_feature_layout():
    from open3dpypro import Feature

    d = np.arange(33 * 5, dtype=np.float64).reshape(33, 5)
    f = Feature(data=d)
    assert (f.dimension(), f.num()) == (33, 5) and f.data is d


def test_fpfh_argument_errors_need_no_gpu():
    from open3dpypro import KDTreeSearchParamHybrid, KDTreeSearchParamKNN, KDTreeSearchParamRadius

    pc = _cloud(10, normals=True)
    with pytest.raises(ValueError, match="64"):
        pc.compute_fpfh_feature(KDTreeSearchParamHybrid(0.1, 65))
    with pytest.raises(ValueError, match="64"):
        pc.compute_fpfh_feature(KDTreeSearchParamKNN(100))
    with pytest.raises(NotImplementedError):
        pc.compute_fpfh_feature(KDTreeSearchParamRadius(0.1))
    with pytest.raises(RuntimeError, match="normal"):
        _cloud(10).compute_fpfh_feature(KDTreeSearchParamHybrid(0.1, 30))
    from open3dpypro import PointCloud

    wide = PointCloud(np.float64([[1e9 + 0.125, 0, 0], [1e9 + 0.25, 1, 0], [1e9 + 0.375, 0, 1]]),
                      normals=np.tile(np.float32([0, 0, 1]), (3, 1)))
    with pytest.raises(NotImplementedError, match="float64"):
        wide.compute_fpfh_feature(KDTreeSearchParamHybrid(0.1, 30))


def test_ransac_argument_errors_and_empty_results_need_no_gpu():
    from open3dpypro import (CorrespondenceCheckerBasedOnDistance, Feature, TransformationEstimationPointToPlane,
                             TransformationEstimationPointToPoint)

    a, b = _cloud(10), _cloud(12)
    corres = np.int32([[0, 1], [1, 2], [2, 3], [3, 4]])

    def empty(r):
        return (np.array_equal(r.transformation, np.eye(4)) and r.fitness == 0.0 and r.inlier_rmse == 0.0
                and len(r.correspondence_set) == 0)

    assert empty(a.registration_ransac_based_on_correspondence(b, corres, 0.1, ransac_n=2))
    assert empty(a.registration_ransac_based_on_correspondence(b, corres[:2], 0.1))
    assert empty(a.registration_ransac_based_on_correspondence(b, corres, 0.0))
    assert empty(a.registration_ransac_based_on_correspondence(b, corres, -1.0,
                                                               checkers=[CorrespondenceCheckerBasedOnDistance(0.1)]))
    with pytest.raises(ValueError):
        a.registration_ransac_based_on_correspondence(b, corres, 0.1, TransformationEstimationPointToPlane())
    with pytest.raises(ValueError):
        a.registration_ransac_based_on_correspondence(b, corres, 0.1, TransformationEstimationPointToPoint(True))

    class Normal:
        normal_angle_threshold = 0.1

    with pytest.raises(ValueError):
        a.registration_ransac_based_on_correspondence(b, corres, 0.1, checkers=[Normal()])
    fa, fb = Feature(data=np.zeros((33, 10))), Feature(data=np.zeros((33, 12)))
    assert empty(a.registration_ransac_based_on_feature_matching(b, fa, fb, True, 0.1, ransac_n=2))
    assert empty(a.registration_ransac_based_on_feature_matching(b, fa, fb, False, 0.0))
    with pytest.raises(ValueError):
        a.registration_ransac_based_on_feature_matching(b, fa, fb, True, 0.1, TransformationEstimationPointToPlane())


def test_new_symbols_are_declared_and_built():
    from open3dpypro import _native as N

    lib = N.load()
    for s in ("o3dx_fpfh", "o3dx_fpfh_workspace_bytes", "o3dx_feature_match", "o3dx_feature_match_workspace_bytes",
              "o3dx_umeyama_from_samples", "o3dx_corr_check", "o3dx_corr_count", "o3dx_corr_count_workspace_bytes",
              "o3dx_corr_error2"):
        assert s in N.declared_symbols() and hasattr(lib, s)
        assert s + "(" in open(N.HEADER_PATH).read()
