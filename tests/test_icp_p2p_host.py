"""Point-to-point ICP (Umeyama, optional scaling): the host side — symbols,
the 3x3 Jacobi-SVD solve against numpy, argument checks and the Python
surface.  Runs without a GPU.

The numpy restatement of Open3D 0.19's RegistrationICP with
TransformationEstimationPointToPoint(with_scaling) lives here (np_umeyama,
np_p2p_sums, np_registration_icp_p2p); tests/test_gpu_icp_p2p.py imports it.
"""
import ctypes

import numpy as np
import pytest

import open3dpypro as o3p
from open3dpypro import _native as N
from open3dpypro import ops, synthetic as S

SHIFT = np.array([12345.678, 23456.789, 98.765])


# ------------------------------------------------------ numpy restatement
def np_umeyama(P, Q, with_scaling=False):
    """Eigen::umeyama(P, Q, with_scaling) (Eigen 3.4) as a 4x4 [cR | t]: the
    demeaned form, SVD by np.linalg.svd.  No pairs: the identity."""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    n = len(P)
    if n == 0:
        return np.eye(4)
    pm, qm = P.mean(0), Q.mean(0)
    dp, dq = P - pm, Q - qm
    sigma = dq.T @ dp / n
    U, s, Vt = np.linalg.svd(sigma)
    Sd = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        Sd[2] = -1
    R = U @ np.diag(Sd) @ Vt
    c = 1.0
    if with_scaling:
        c = float(s @ Sd) / ((dp * dp).sum() / n)
    T = np.eye(4)
    T[:3, :3] = c * R
    T[:3, 3] = qm - c * R @ pm
    return T


def np_p2p_sums(P, Q, anchor):
    """The library's point-to-point sums vector (include/o3dx.h) of matched
    pairs (P already transformed), in numpy float64, about `anchor`."""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    a = np.asarray(anchor, np.float64)
    p, q = P - a, Q - a
    sums = np.zeros(32)
    sums[0:9] = (q.T @ p).ravel()
    sums[9:12] = p.sum(0)
    sums[12:15] = q.sum(0)
    sums[15] = (p * p).sum()
    sums[16:19] = a
    sums[28] = len(P)
    sums[29] = ((P - Q) ** 2).sum()
    return sums


def np_transform(T, X):
    """Open3D's in-place pcd.Transform: ((t0 x + t1 y) + t2 z) + t3 per row."""
    X = np.asarray(X, np.float64)
    return np.stack([((T[r, 0] * X[:, 0] + T[r, 1] * X[:, 1]) + T[r, 2] * X[:, 2]) + T[r, 3] for r in range(3)], 1)


def np_registration_icp_p2p(src, tgt, max_corr, with_scaling=False, init=None, max_iteration=30,
                            relative_fitness=1e-6, relative_rmse=1e-6, knn1=None):
    """Open3D RegistrationICP with TransformationEstimationPointToPoint: the
    source is transformed in place by every update (the cumulative form);
    correspondences = 1-NN with d < max_corr (knn1(points) -> (idx, d2), -1
    for none; default: the oracle's KDTree restatement).
    -> (T, fitness, rmse, corr (m,2))."""
    if knn1 is None:
        from oracle import oracle as O

        def knn1(q):
            idx, d2, cnt = O.knn_search(tgt, q, O.HYBRID, 1, max_corr)
            return np.where(cnt > 0, idx[:, 0], -1), d2[:, 0]
    tgt64 = np.asarray(tgt, np.float64)
    T = np.eye(4) if init is None else np.array(init, np.float64)
    pts = np_transform(T, src)

    def evaluate(p):
        j, _ = knn1(p)
        i = np.nonzero(j >= 0)[0]
        j = j[i]
        d2 = ((p[i] - tgt64[j]) ** 2).sum(1)
        if len(i) == 0:
            return i, j, 0.0, 0.0
        return i, j, len(i) / len(p), float(np.sqrt(d2.sum() / len(i)))

    i, j, fit, rm = evaluate(pts)
    for _ in range(max_iteration):
        upd = np_umeyama(pts[i], tgt64[j], with_scaling)
        T = upd @ T
        pts = np_transform(upd, pts)
        pf, pr = fit, rm
        i, j, fit, rm = evaluate(pts)
        if abs(pf - fit) < relative_fitness and abs(pr - rm) < relative_rmse:
            break
    return T, fit, rm, np.stack([i, j], 1)


# ------------------------------------------------------------ the sets
def _random_rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _sets(count=200, seed=7):
    """Correspondence sets (P, Q, kind) as ICP meets them — Q within reach of
    P, both inside one box whose corner is the anchor: generic anisotropic
    clouds turned about their centroid, scaled, shifted a little and
    perturbed; and noisy near-planar sets whose Q is the mirror image of P
    across the plane, so the best orthogonal map is a reflection and Umeyama
    takes its S = diag(1, 1, -1) branch.

    The sums vector is float64: forming the covariance from sums about an
    anchor at distance D cancels to an absolute error of about 2^-52 D^2,
    which the rotation sees divided by the smallest singular value s2 (for a
    reflection, by s1 - s2 as well).  Here D^2 <~ 4 and s2 >~ 2e-3 (a
    thickness of 5 % of the extent or more), a floor of about 4e-13: the sets
    keep the 1e-12 bar meaningful for the solve itself."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        n = int(rng.integers(8, 400))
        ext = np.array([1.0, rng.uniform(0.3, 1.0), rng.uniform(0.2, 1.0)])
        P = (rng.random((n, 3)) - 0.5) * ext
        kind = "generic"
        if k % 3 == 2:
            kind = "mirror"
            P[:, 2] = rng.normal(scale=rng.uniform(0.05, 0.15), size=n)
        P = P @ _random_rotation(rng).T + rng.uniform(-0.2, 0.2, 3)
        c = P.mean(0)
        X = P
        if kind == "mirror":  # mirrored across the plane through the centroid, before the motion
            nrm = np.linalg.svd((P - c).T @ (P - c))[0][:, 2]
            X = P - 2 * np.outer((P - c) @ nrm, nrm)
        R = _random_rotation(rng)
        Q = (rng.uniform(0.8, 1.25) * ((X - c) @ R.T) + c + rng.uniform(-0.1, 0.1, 3)
             + rng.normal(scale=1e-3, size=(n, 3)))
        out.append((P, Q, kind))
    return out


def _sv(P, Q):
    dp, dq = P - P.mean(0), Q - Q.mean(0)
    U, s, Vt = np.linalg.svd(dq.T @ dp / len(P))
    return s, np.linalg.det(U) * np.linalg.det(Vt)


# ------------------------------------------------------------------ tests
def test_p2p_symbols_declared_and_exported():
    lib = N.load()
    new = ["o3dx_icp_target_build_points", "o3dx_icp_target_build_points_f64", "o3dx_icp_accumulate_est",
           "o3dx_icp_register_est", "o3dx_icp_register_est_f64", "o3dx_registration_icp_est",
           "o3dx_registration_icp_est_f64", "o3dx_icp_solve_point_to_point", "o3dx_icp_update_est"]
    hdr = open(N.HEADER_PATH).read()
    for name in new:
        assert name in N.declared_symbols(), name
        assert hasattr(lib, name), name
        assert name + "(" in hdr, name
    assert "#define O3DX_ICP_POINT_TO_PLANE 0" in hdr and "#define O3DX_ICP_POINT_TO_POINT 1" in hdr
    assert (N.ICP_POINT_TO_PLANE, N.ICP_POINT_TO_POINT) == (0, 1)
    assert lib.o3dx_abi_version() == 7


@pytest.mark.parametrize("with_scaling", [False, True])
def test_p2p_solve_matches_numpy_umeyama(with_scaling):
    """o3dx_icp_solve_point_to_point on numpy-built sums equals the numpy
    Umeyama within 1e-12, over ~200 sets with singular-value ratios <= 1e3 as
    numpy reports them (a Jacobi SVD's error is a few ulp times that ratio:
    1e3 x 2.2e-16 x a few, far below 1e-12 on these O(1) coordinates),
    reflections (S = -1) included."""
    used = mirrored = 0
    worst = 0.0
    for P, Q, kind in _sets():
        s, dd = _sv(P, Q)
        if not s[0] / s[2] <= 1e3:
            continue
        used += 1
        mirrored += dd < 0
        anchor = np.minimum(P.min(0), Q.min(0)) - 0.05  # the box corner, as the target grid's origin is
        upd, rc = ops.icp_solve_point_to_point(np_p2p_sums(P, Q, anchor), with_scaling, return_status=True)
        ref = np_umeyama(P, Q, with_scaling)
        assert rc == 1
        worst = max(worst, np.abs(upd - ref).max())
        np.testing.assert_allclose(upd, ref, rtol=0, atol=1e-12, err_msg=kind)
        assert np.array_equal(upd[3], [0, 0, 0, 1])
    print(f"sets {used}, reflections {mirrored}, max |update - numpy| {worst:.2e}")
    assert used >= 150 and mirrored >= 30


@pytest.mark.parametrize("with_scaling", [False, True])
def test_p2p_solve_anchor_shift(with_scaling):
    """A set and its anchor shifted by (12345.678, 23456.789, 98.765): the
    anchored sums are those of the unshifted set up to the rounding of the
    shifted coordinates (4e-12 each), so the same update results within 1e-9:
    the same motion of the cloud, compared in the cloud's own frame (Shift^-1
    U Shift against the unshifted U — in the world frame the translation of a
    rotation about a point 2.7e4 away magnifies the inputs' rounding by that
    distance, for numpy's Umeyama alike), and the numpy Umeyama of the same
    shifted set in the world frame."""
    Sh, Shi = np.eye(4), np.eye(4)
    Sh[:3, 3], Shi[:3, 3] = SHIFT, -SHIFT
    for P, Q, _ in _sets(20, seed=3):
        s, _ = _sv(P, Q)
        if not s[0] / s[2] <= 1e3:
            continue
        a = np.minimum(P.min(0), Q.min(0)) - 0.05
        u0 = ops.icp_solve_point_to_point(np_p2p_sums(P, Q, a), with_scaling)
        Ps, Qs = P + SHIFT, Q + SHIFT
        u1 = ops.icp_solve_point_to_point(np_p2p_sums(Ps, Qs, a + SHIFT), with_scaling)
        np.testing.assert_allclose(Shi @ u1 @ Sh, u0, rtol=0, atol=1e-9)
        np.testing.assert_allclose(u1, np_umeyama(Ps, Qs, with_scaling), rtol=0, atol=1e-9)


def test_p2p_solve_degenerate():
    rng = np.random.default_rng(0)
    # no correspondences: the identity, 0
    for ws in (False, True):
        upd, rc = ops.icp_solve_point_to_point(np.zeros(32), ws, return_status=True)
        assert rc == 0 and np.array_equal(upd, np.eye(4))
    # a source of zero spread with scaling (var_p = 0): the identity, 0
    P = np.tile([[0.5, -0.25, 0.75]], (16, 1))  # (binary fractions: the sums, and so var_p = 0, are exact)
    Q = rng.random((16, 3))
    upd, rc = ops.icp_solve_point_to_point(np_p2p_sums(P, Q, [0, 0, 0]), True, return_status=True)
    assert rc == 0 and np.array_equal(upd, np.eye(4))
    # exactly planar correspondences (z = 0 in both clouds): the third singular
    # value is 0, the rotation still proper and orthogonal
    ang = 0.4
    Rz = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
    P = np.c_[rng.random((50, 2)), np.zeros(50)]
    Q = P @ Rz.T + [0.1, -0.3, 0.0]
    for anchor in ([0, 0, 0], [-0.25, -0.5, -0.125], [-0.1, -0.3, -0.7]):
        for ws in (False, True):
            upd, rc = ops.icp_solve_point_to_point(np_p2p_sums(P, Q, anchor), ws, return_status=True)
            R = upd[:3, :3]
            assert rc == 1
            assert abs(np.linalg.det(R) - 1) < 1e-12
            np.testing.assert_allclose(R.T @ R, np.eye(3), rtol=0, atol=1e-12)
            np.testing.assert_allclose(upd[:3, :3], Rz, rtol=0, atol=1e-12)
            np.testing.assert_allclose(upd[:3, 3], [0.1, -0.3, 0.0], rtol=0, atol=1e-12)


def test_p2p_host_update_equals_solve_times_T():
    P, Q, _ = _sets(1, seed=5)[0]
    sums = np_p2p_sums(P, Q, P.min(0))
    T0 = S.rigid_transform(3.0)
    for ws in (False, True):
        T1 = ops.icp_update(sums, T0, estimation="point_to_point", with_scaling=ws)
        assert np.allclose(T1, ops.icp_solve_point_to_point(sums, ws) @ T0, rtol=0, atol=1e-15)
    # the default estimation is still point-to-plane
    pl = np.zeros(32)
    pl[[0, 6, 11, 15, 18, 20]] = 1.0
    pl[21:27] = [0, 0, -0.01, -0.1, 0.2, -0.3]
    pl[28] = 5
    assert np.array_equal(ops.icp_update(pl, T0), ops.icp_update(pl, T0, estimation="point_to_plane"))
    assert np.allclose(ops.icp_update(pl, T0), ops.icp_solve(pl) @ T0, atol=1e-15)
    with pytest.raises(ValueError):
        ops.icp_update(sums, T0, estimation="point_to_line")


def test_p2p_entries_validate_before_touching_the_device():
    """Every new entry returns -EINVAL for an unknown estimation, and the
    point-to-plane entries refuse a descriptor with the no-normals flag, before
    any device call (so this runs without a GPU)."""
    L = N.load()
    v = ctypes.c_void_p(8)  # never dereferenced: the checks come first
    desc = np.zeros(N.ICP_DESC_LEN)
    dp = desc.ctypes.data_as(ctypes.c_void_p)
    T = np.eye(4)
    Tp = T.ctypes.data_as(ctypes.c_void_p)
    sums = np.zeros(32)
    sp = sums.ctypes.data_as(ctypes.c_void_p)
    for bad in (2, -1, 7):
        calls = {
            "accumulate_est": L.o3dx_icp_accumulate_est(v, 10, 0, v, dp, Tp, 0.1, None, sp, None, None, None, bad,
                                                        v, 1 << 30, None),
            "register_est": L.o3dx_icp_register_est(v, 10, 0, v, dp, None, 3, 0.0, 0.0, 0.1, None, v, v, v, None,
                                                    None, bad, 0, v, 1 << 30, None),
            "register_est_f64": L.o3dx_icp_register_est_f64(v, 10, 0, v, dp, None, 3, 0.0, 0.0, 0.1, None, v, v, v,
                                                            None, None, bad, 0, v, 1 << 30, None),
            "registration_icp_est": L.o3dx_registration_icp_est(v, 10, v, None, 10, 0.1, None, 3, 0.0, 0.0, v, v, v,
                                                                None, None, bad, 0, v, 1 << 30, v, 1 << 30, None),
            "registration_icp_est_f64": L.o3dx_registration_icp_est_f64(v, 10, v, None, 10, 0.1, None, 3, 0.0, 0.0,
                                                                        v, v, v, None, None, bad, 0, v, 1 << 30, v,
                                                                        1 << 30, None),
            "update_est": L.o3dx_icp_update_est(sp, bad, 0, Tp),
        }
        for name, rc in calls.items():
            assert rc == -22, (name, bad, rc)
        assert b"estimation" in L.o3dx_last_error()
    assert np.array_equal(T, np.eye(4))
    # a hand-made descriptor: the magic and the no-normals flag
    desc[13] = 4242.0
    desc[19] = 1.0
    fit, rm = np.zeros(1), np.zeros(1)
    rc = L.o3dx_icp_register(None, 0, 0, v, dp, None, 3, 0.0, 0.0, 0.1, None, Tp,
                             fit.ctypes.data_as(ctypes.c_void_p), rm.ctypes.data_as(ctypes.c_void_p), None, None, v,
                             1 << 30, None)
    assert rc == -22 and b"normals" in L.o3dx_last_error()
    rc = L.o3dx_icp_accumulate(None, 0, 0, v, dp, Tp, 0.1, None, sp, None, None, None, v, 1 << 30, None)
    assert rc == -22 and b"normals" in L.o3dx_last_error()
    rc = L.o3dx_icp_register_est(None, 0, 0, v, dp, None, 3, 0.0, 0.0, 0.1, None, Tp,
                                 fit.ctypes.data_as(ctypes.c_void_p), rm.ctypes.data_as(ctypes.c_void_p), None, None,
                                 N.ICP_POINT_TO_PLANE, 0, v, 1 << 30, None)
    assert rc == -22 and b"normals" in L.o3dx_last_error()


def test_p2p_python_surface():
    from open3dpypro import params
    pipes = [o3p.Processors.ICP(max_correspondence_distance=0.05, estimation="point_to_point", with_scaling=True),
             o3p.Processors.ICP(max_correspondence_distance=0.05)]
    back = o3p.PointCloudMatProcessors.loads(o3p.PointCloudMatProcessors.dumps(pipes))
    assert back[0].estimation == "point_to_point" and back[0].with_scaling is True
    assert back[1].estimation == "point_to_plane" and back[1].with_scaling is False
    assert back[0].uuid == pipes[0].uuid
    src = o3p.PointCloud(np.random.rand(20, 3))
    tgt = o3p.PointCloud(np.random.rand(20, 3))
    with pytest.raises(ValueError):
        src.registration_icp(tgt, 0.1, estimation="bogus")
    with pytest.raises(ValueError):
        src.registration_icp(tgt, 0.1, estimation=params.KDTreeSearchParamKNN(3))
    # point-to-plane (the default) still needs target normals
    with pytest.raises(RuntimeError, match="normal"):
        src.registration_icp(tgt, 0.1)
    assert params.resolve_estimation("point_to_point") == ("point_to_point", False)
    assert params.resolve_estimation(params.TransformationEstimationPointToPoint(True)) == ("point_to_point", True)
    assert params.resolve_estimation(params.TransformationEstimationPointToPoint()) == ("point_to_point", False)
    assert params.resolve_estimation(params.TransformationEstimationPointToPlane()) == ("point_to_plane", False)
    # a target without normals validates for point-to-point only
    from open3dpypro.PointCloudMat import PointCloudMat, ShapeType
    m = PointCloudMat(shape_type=ShapeType.XYZ).build(np.random.rand(10, 3).astype(np.float32))
    o3p.Processors.ICP(estimation="point_to_point").validate_pcd(1, m)
    with pytest.raises(TypeError):
        o3p.Processors.ICP().validate_pcd(1, m)
