"""ISS keypoints and the radius outlier filter without a GPU: the oracle
against a second restatement, the fixtures against the generator, and the
host-side surface (Feature.select_by_index, argument checks, empty clouds)."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import iss_oracle as O  # noqa: E402
import make_iss_golden as G  # noqa: E402


@pytest.fixture(scope="module")
def clouds():
    return G.load_clouds()


def _plain_iss(P, sr, nr, g21, g32, mn):
    """The rules once more, a point at a time with nothing shared."""
    P = P.astype(np.float64)
    n = len(P)
    s = np.zeros(n)
    cnt = np.zeros(n, np.int32)
    nbr_nr = []
    for i in range(n):
        d = P[i] - P
        d2 = ((d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        nbr_nr.append(np.nonzero(d2 < nr * nr)[0])
        idx = np.nonzero(d2 < sr * sr)[0]
        cnt[i] = len(idx)
        if len(idx) < mn:
            continue
        C = np.cov(P[idx].T, bias=True)
        if np.all(np.abs(C) <= 1e-12):
            continue
        w = np.sort(np.linalg.eigvalsh(C))[::-1]
        if w[1] / w[0] < g21 and w[2] / w[1] < g32:
            s[i] = w[2]
    kp = [i for i in range(n)
          if s[i] > 0 and len(nbr_nr[i]) >= mn and not (s[i] < s[nbr_nr[i]]).any()]
    return s, cnt, np.asarray(kp, np.int64)


def test_oracle_against_a_plain_loop(clouds):
    P = clouds["cube"][:1200]  # the first 1200 points: ~9 neighbours at 0.12, every branch taken
    sr, nr, g21, g32, mn = 0.12, 0.1, 0.9, 0.9, 5
    r = O.iss(P, sr, nr, g21, g32, mn)
    s, cnt, kp = _plain_iss(P, sr, nr, g21, g32, mn)
    assert np.array_equal(r["count"], cnt)
    assert (cnt < mn).any() and (cnt >= mn).any() and (s == 0)[cnt >= mn].any()
    assert np.array_equal(r["s"] != 0, s != 0)
    # np.cov centres the same way; the two agree to rounding of |C|
    assert np.abs(r["s"] - s).max() <= 1e-13 * r["e1"].max()
    con = r["contested"]
    assert not con.any()
    assert np.array_equal(r["keypoints"], kp) and len(kp) > 0


def test_neighbor_lists_equal_brute_force(clouds):
    P = clouds["cube"][:1500].astype(np.float64)
    for rad in (0.05, 0.12):
        a = O.neighbors(P, rad)
        b = O.neighbors_brute(P, rad)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # the rule is strict: a lattice has pairs at exactly d^2 = r^2
    g = np.stack(np.meshgrid(*[np.arange(4) * 0.125] * 3, indexing="ij"), -1).reshape(-1, 3)
    ptr, ind = O.neighbors(g, 0.25)
    bp, bi = O.neighbors_brute(g, 0.25)
    assert np.array_equal(ptr, bp) and np.array_equal(ind, bi)
    d2 = O._d2(g[:, None, :], g[None, :, :])
    assert (d2 == 0.0625).any() and np.array_equal(np.diff(ptr), (d2 < 0.0625).sum(1))


@pytest.mark.parametrize("name", ["sphere_auto", "sphere_r", "cube_auto", "cube_r", "wide_auto", "dups_r",
                                  "bunny_r005"])
def test_fixture_reproduces(clouds, name):
    cloud, params = G.CASES[name]
    want = G.load_case(name)
    got = G.run_case(clouds[cloud], params)
    for f in G.FIELDS:
        assert np.array_equal(got[f], want[f]), f
    assert want["contested"].sum() <= G.MAX_CONTESTED * len(clouds[cloud])


def test_fixture_numbers():
    """What the issue recorded for the clouds that are a function of bunny.pcd."""
    for name, kp, con in (("bunny_auto", 343, 2), ("bunny_r005", 280, 2), ("bunny_big", 50, 0), ("wide_auto", 148, 0)):
        c = G.load_case(name)
        assert (len(c["keypoints"]), int(c["contested"].sum())) == (kp, con), name
    assert int(G.load_case("bunny_big")["count"].max()) == 390
    c = G.load_case("cube_r")
    assert (c["count"] == 5).any() and (c["count"] < 5).any()


def test_dups_keypoints_come_in_pairs():
    c = G.load_case("dups_r")
    kp = c["keypoints"]
    assert len(kp) > 0 and len(kp) % 2 == 0
    assert (kp[0::2] % 2 == 0).all() and np.array_equal(kp[0::2] + 1, kp[1::2])
    assert np.array_equal(c["s"][0::2], c["s"][1::2])  # bit-equal: the same neighbour set


def test_feature_select_by_index_host():
    from open3dpypro import Feature

    data = np.arange(33 * 7, dtype=np.float64).reshape(33, 7)
    f = Feature(data=data)
    g = f.select_by_index([5, 1, 1])
    assert (g.dimension(), g.num()) == (33, 2) and np.array_equal(g.data, data[:, [1, 5]])
    g = f.select_by_index(np.array([5, 1]), invert=True)
    assert np.array_equal(g.data, data[:, [0, 2, 3, 4, 6]])
    e = f.select_by_index([])
    assert (e.dimension(), e.num()) == (33, 0) and e.data.shape == (33, 0)
    assert np.array_equal(f.select_by_index([], invert=True).data, data)
    with pytest.raises(IndexError):
        f.select_by_index([7])
    assert f.data is data  # the source is untouched


def test_argument_validation():
    from open3dpypro import PointCloud

    pc = PointCloud(np.random.default_rng(0).random((50, 3)).astype(np.float32))
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            pc.compute_iss_keypoints(salient_radius=bad, non_max_radius=0.1)
        with pytest.raises(ValueError):
            pc.get_index_by_iss_keypoints(salient_radius=0.1, non_max_radius=bad)
        with pytest.raises(ValueError):
            pc.remove_radius_outlier(3, bad)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            pc.compute_iss_keypoints(0.1, 0.1, gamma_21=bad)
        with pytest.raises(ValueError):
            pc.compute_iss_keypoints(0.1, 0.1, gamma_32=bad)
    pts = np.random.default_rng(0).random((50, 3)).astype(np.float32)
    pts[17, 1] = np.nan
    nan_pc = PointCloud(pts)
    with pytest.raises(ValueError):
        nan_pc.compute_iss_keypoints(0.1, 0.1)
    with pytest.raises(ValueError):
        nan_pc.remove_radius_outlier(3, 0.1)


def test_empty_cloud_returns():
    import open3dpypro
    from open3dpypro import PointCloud

    pc = PointCloud()
    out = pc.compute_iss_keypoints()
    assert isinstance(out, PointCloud) and out.size() == 0
    assert open3dpypro.compute_iss_keypoints(pc).size() == 0
    assert open3dpypro.keypoint.compute_iss_keypoints(pc, 0.1, 0.1).size() == 0
    idx = pc.get_index_by_iss_keypoints()
    assert idx.dtype == np.int64 and idx.shape == (0,)
    cloud, kept = pc.remove_radius_outlier(3, 0.1)
    assert cloud.size() == 0 and kept == []
