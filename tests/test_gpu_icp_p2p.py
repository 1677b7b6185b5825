"""Point-to-point ICP (Umeyama, optional scaling) on the device loop, against
the numpy restatement of Open3D's RegistrationICP +
TransformationEstimationPointToPoint in tests/test_icp_p2p_host.py."""
import functools

import numpy as np
import pytest
import torch

import open3dpypro as o3p
from oracle import oracle as O
from open3dpypro import _native as N
from open3dpypro import ops, synthetic as S
from open3dpypro.PointCloudMat import PointCloudMat, ShapeType
from test_icp_p2p_host import np_p2p_sums, np_registration_icp_p2p, np_transform

pytestmark = pytest.mark.gpu

P2P = "point_to_point"
MC = 0.02
OFF = (12345.678, 23456.789, 98.765)


@functools.lru_cache(maxsize=None)
def _icp_case(n, seed=1):
    tgt = S.box_surface(n, seed)
    src = S.apply_transform(S.box_surface(n, seed + 1), S.rigid_transform())
    return src.numpy(), tgt.numpy()


@functools.lru_cache(maxsize=None)
def _reference(n, with_scaling):
    src, tgt = _icp_case(n)
    return np_registration_icp_p2p(src, tgt, MC, with_scaling, max_iteration=30, relative_fitness=0.0,
                                   relative_rmse=0.0)


def _sorted_pairs(corr):
    c = corr.cpu().numpy().astype(np.int64)
    return c[np.argsort(c[:, 0])]


def test_p2p_accumulate_matches_numpy(dev):
    """n = 33001: 129 blocks (the 128 accumulator copies wrap) and a partial
    last wave.  The count and the correspondence set equal the oracle's, the
    16 anchored moments numpy's (the bar of test_icp_accumulate_matches_oracle),
    and the fx rows do not depend on the source's order."""
    n = 33001
    src, tgt = _icp_case(n)
    T = S.rigid_transform(0.3, (0, 0, 1), (0.001, 0, 0))
    target = ops.ICPTarget(torch.from_numpy(tgt).to(dev), None, MC)
    s = torch.from_numpy(src).to(dev)
    sums, corr, fx = target.accumulate(s, T, want_corr=True, return_fx=True, estimation=P2P)
    q = np_transform(T, src)
    ridx, _, rc = O.knn_search(tgt, q, O.HYBRID, 1, MC)
    exp = np.stack([np.nonzero(rc > 0)[0], ridx[rc > 0, 0]], 1)
    assert np.array_equal(_sorted_pairs(corr), exp)
    anchor = sums[16:19].copy()
    assert np.array_equal(anchor, target.desc[0:3])  # the target grid's origin
    assert np.all(anchor <= tgt.min(0))
    ref = np_p2p_sums(q[exp[:, 0]], tgt[exp[:, 1]].astype(np.float64), anchor)
    assert sums[28] == ref[28] == len(exp)
    np.testing.assert_allclose(sums[:16], ref[:16], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(sums[29], ref[29], rtol=1e-9, atol=1e-9)
    assert not sums[19:28].any() and not sums[30:].any()
    assert not fx[16:28, :2].any()  # the anchor's and the unused slots' digits are 0
    sums4, corr4, fx4 = target.accumulate(ops.spatial_sort(s), T, want_corr=True, return_fx=True, estimation=P2P)
    assert np.array_equal(fx4, fx) and np.array_equal(sums4, sums)
    assert torch.equal(corr4, corr)


@pytest.mark.parametrize("with_scaling", [False, True])
@pytest.mark.parametrize("n", [30000, 5000])
def test_p2p_registration_parity(dev, n, with_scaling):
    """30 iterations, no early stop: T within 1e-5, fitness and rmse within 1e-6
    of the restatement (n = 5000: fitness ~0.8, a fifth of the lanes add zeros)."""
    src, tgt = _icp_case(n)
    res = ops.registration_icp(torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev), None, MC,
                               max_iteration=30, relative_fitness=0.0, relative_rmse=0.0, estimation=P2P,
                               with_scaling=with_scaling)
    T, fit, rmse, corr = _reference(n, with_scaling)
    print(f"n {n} scaling {with_scaling}: max |T - ref| {np.abs(res['transformation'] - T).max():.2e}, fitness "
          f"{res['fitness']:.6f} (ref {fit:.6f}), rmse {res['inlier_rmse']:.3e} (ref {rmse:.3e})")
    np.testing.assert_allclose(res["transformation"], T, rtol=0, atol=1e-5)
    assert abs(res["fitness"] - fit) < 1e-6
    assert abs(res["inlier_rmse"] - rmse) < 1e-6
    assert len(res["correspondence_set"]) == len(corr)
    if n == 30000 and not with_scaling:  # the planted motion, to the sampling noise of two samplings of the box
        assert np.abs(res["transformation"] - np.linalg.inv(S.rigid_transform())).max() < 2e-3


@pytest.mark.parametrize("with_scaling", [False, True])
@pytest.mark.parametrize("rel", [0.0, 1e-6])
def test_p2p_device_loop_equals_host_loop(dev, rel, with_scaling):
    """The device loop (k_icp_finish's Umeyama solve) gives T, fitness, rmse
    and the correspondences of the host loop over accumulate + icp_update to
    the bit, with and without an early stop; the one-call registration_icp
    agrees (mirrors test_icp_device_loop_equals_host_loop)."""
    src, tgt = _icp_case(30000, seed=11)
    t = torch.from_numpy(tgt).to(dev)
    target = ops.ICPTarget(t, None, MC)
    s4 = ops.spatial_sort(torch.from_numpy(src).to(dev))
    am = np.abs(src.astype(np.float64)).max(0)
    kw = dict(estimation=P2P, with_scaling=with_scaling)
    res = target.register(s4, max_iteration=25, relative_fitness=rel, relative_rmse=rel, absmax=am, want_corr=True,
                          **kw)
    T = np.eye(4)
    sums, _ = target.accumulate(s4, T, absmax=am, estimation=P2P)
    fit, rm = sums[28] / len(src), np.sqrt(sums[29] / sums[28])
    for _ in range(25):
        T = ops.icp_update(sums, T, **kw)
        pf, pr = fit, rm
        sums, corr = target.accumulate(s4, T, absmax=am, want_corr=True, estimation=P2P)
        fit, rm = sums[28] / len(src), np.sqrt(sums[29] / sums[28])
        if abs(pf - fit) < rel and abs(pr - rm) < rel:
            break
    assert np.array_equal(res["transformation"], T)
    assert res["fitness"] == fit and res["inlier_rmse"] == rm
    assert torch.equal(res["correspondence_set"], corr)
    one = ops.registration_icp(torch.from_numpy(src).to(dev), t, None, MC, max_iteration=25, relative_fitness=rel,
                               relative_rmse=rel, **kw)
    assert np.array_equal(one["transformation"], T) and one["fitness"] == fit and one["inlier_rmse"] == rm
    assert torch.equal(one["correspondence_set"], corr)


def test_p2p_skip_proof_equals_full_search(dev, monkeypatch):
    """The skip proof under the point-to-point update (the proof bounds the
    motion from the positions themselves, so a scaling T is covered): T,
    fitness, rmse and the final correspondences equal the loop that searches
    every step (O3DX_ICP_SKIP=0) to the bit, and fewer queries are searched."""
    n = 300_000
    src, tgt = _icp_case(n, seed=21)
    target = ops.ICPTarget(torch.from_numpy(tgt).to(dev), None, MC)
    s4 = ops.spatial_sort(torch.from_numpy(src).to(dev))
    for ws in (False, True):
        runs = {}
        for mode in ("1", "0"):
            monkeypatch.setenv("O3DX_ICP_SKIP", mode)
            N.search_stats(True)
            res = target.register(s4, max_iteration=30, relative_fitness=0.0, relative_rmse=0.0, want_corr=True,
                                  estimation=P2P, with_scaling=ws)
            runs[mode] = (res, N.search_stats()["queries"])
            N.search_stats(False)
        (a, qa), (b, qb) = runs["1"], runs["0"]
        assert np.array_equal(a["transformation"], b["transformation"])
        assert a["fitness"] == b["fitness"] and a["inlier_rmse"] == b["inlier_rmse"]
        assert torch.equal(a["correspondence_set"], b["correspondence_set"])
        msg = f"with_scaling {ws}: searched queries with skip {qa}, without {qb}, ratio {qa / qb:.3f}"
        print(msg)
        assert qb >= 31 * n and qa < qb, msg


def test_p2p_target_without_normals(dev):
    """A target built without normals gives the point-to-point results of one
    built with normals to the bit and refuses point-to-plane; the PointCloud
    and Processors surfaces take such a target."""
    src, tgt = _icp_case(20000, seed=5)
    s, t = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
    tn = ops.estimate_normals(t, knn=30)
    bare, full = ops.ICPTarget(t, None, MC), ops.ICPTarget(t, tn, MC)
    assert bare.desc[19] == 1 and full.desc[19] == 0
    kw = dict(max_iteration=20, relative_fitness=0.0, relative_rmse=0.0, want_corr=True, estimation=P2P)
    a, b = bare.register(s, **kw), full.register(s, **kw)
    assert np.array_equal(a["transformation"], b["transformation"])
    assert a["fitness"] == b["fitness"] and a["inlier_rmse"] == b["inlier_rmse"]
    assert torch.equal(a["correspondence_set"], b["correspondence_set"])
    T = S.rigid_transform(0.2, (1, 0, 0), (0, 0.002, 0))
    sa, _, fa = bare.accumulate(s, T, return_fx=True, estimation=P2P)
    sb, _, fb = full.accumulate(s, T, return_fx=True, estimation=P2P)
    assert np.array_equal(fa, fb) and np.array_equal(sa, sb)
    with pytest.raises(RuntimeError, match="normals"):
        bare.register(s, max_iteration=2)
    with pytest.raises(RuntimeError, match="normals"):
        bare.accumulate(s, T)
    with pytest.raises(RuntimeError, match="normals"):
        ops.registration_icp(s, t, None, MC, max_iteration=2)
    # PointCloud: a target without normals, the estimation as a string or an object
    one = ops.registration_icp(s, t, None, MC, max_iteration=20, relative_fitness=0.0, relative_rmse=0.0,
                               estimation=P2P)
    ps, pt = o3p.PointCloud(src), o3p.PointCloud(tgt)
    assert not pt.has_normals()
    for est in (P2P, o3p.params.TransformationEstimationPointToPoint()):
        r = ps.registration_icp(pt, MC, max_iteration=20, relative_fitness=0.0, relative_rmse=0.0, estimation=est)
        assert np.array_equal(r.transformation, one["transformation"])
        assert r.fitness == one["fitness"] and r.inlier_rmse == one["inlier_rmse"]
        assert len(r.correspondence_set) == len(one["correspondence_set"])
    with pytest.raises(RuntimeError, match="normal"):
        ps.registration_icp(pt, MC)
    # Processors.ICP on an XYZ target
    icp = o3p.Processors.ICP(max_correspondence_distance=MC, max_iteration=20, relative_fitness=0.0,
                             relative_rmse=0.0, estimation=P2P)
    out, meta = icp.validate([PointCloudMat(shape_type=ShapeType.XYZ).build(s),
                              PointCloudMat(shape_type=ShapeType.XYZ).build(t)], {})
    assert np.array_equal(np.asarray(meta[icp.uuid]["transformation"]), one["transformation"])
    assert out[0].data().shape == (len(src), 3)
    with pytest.raises(TypeError):
        o3p.Processors.ICP(max_correspondence_distance=MC).validate(
            [PointCloudMat(shape_type=ShapeType.XYZ).build(s), PointCloudMat(shape_type=ShapeType.XYZ).build(t)], {})


@functools.lru_cache(maxsize=None)
def _las_case():
    M = S.rigid_transform(1.0, t=(0.2, -0.12, 0.08))
    tgt = S.las_scene(20000, seed=0, offset=OFF).numpy()
    src = S.las_scene(20000, seed=1, T=M, offset=OFF).numpy()
    ref = {ws: np_registration_icp_p2p(src, tgt, 0.8, ws, max_iteration=30, relative_fitness=0.0, relative_rmse=0.0)
           for ws in (False, True)}
    return src, tgt, ref


@pytest.mark.parametrize("with_scaling", [False, True])
@pytest.mark.parametrize("form", ["unsorted", "sorted_f64", "one_call"])
def test_p2p_f64(dev, form, with_scaling):
    """float64 clouds 1e4 m from the origin (moments about the frame origin,
    not the coordinate origin): T within 1e-5, fitness and rmse within 1e-6 of
    the restatement, for an unsorted and a spatial_sort_f64 source on a built
    target and for the one-call form."""
    src, tgt, ref = _las_case()
    T, fit, rmse, _ = ref[with_scaling]
    s, t = torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev)
    kw = dict(max_iteration=30, relative_fitness=0.0, relative_rmse=0.0, estimation=P2P, with_scaling=with_scaling)
    if form == "one_call":
        res = ops.registration_icp(s, t, None, 0.8, return_corr=False, **kw)
    else:
        target = ops.ICPTarget(t, None, 0.8)
        assert target.f64 and target.desc[19] == 1
        res = target.register(s if form == "unsorted" else ops.spatial_sort_f64(s), **kw)
    print(f"{form} scaling {with_scaling}: max |T - ref| {np.abs(res['transformation'] - T).max():.2e}, fitness "
          f"{res['fitness']:.6f} (ref {fit:.6f}), rmse {res['inlier_rmse']:.3e} (ref {rmse:.3e})")
    np.testing.assert_allclose(res["transformation"], T, rtol=0, atol=1e-5)
    assert abs(res["fitness"] - fit) < 1e-6 and abs(res["inlier_rmse"] - rmse) < 1e-6
