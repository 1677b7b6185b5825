"""RANSAC plane segmentation (o3dx_segment_plane[_f64], o3dx_plane_count[_upper,
_f64], o3dx_plane_abs_sum, o3dx_plane_inliers, o3dx_plane_select[_f64],
PointCloud.seg_planes) on the degenerate clouds of edge_clouds.py and at exact
thresholds: flat, collinear and coincident clouds, lattices with points at
|d| == thr, clouds of ransac_n points, hypotheses that are all degenerate, an
early-stop quotient that underflows, and every upper-bound sweep forced in
turn.

The cases and the plain references are tests/plane_edge_cases.py;
test_plane_edge_cases.py shows on the CPU that the references agree with the
oracle and which cases may be compared bit for bit (selection pinned) and at a
tolerance (refit conditioned)."""
import numpy as np
import pytest
import torch

import edge_clouds as E
import open3dpypro as o3p
import plane_edge_cases as PC
from open3dpypro import ops
from oracle import oracle as O

pytestmark = pytest.mark.gpu

F32 = PC.clouds(wide=False)
F64 = PC.clouds(wide=True)
# (O3DX_RANSAC_UPPER, O3DX_RANSAC_HOST_SETUP): the sweep a call takes on its
# own, then each one forced; the culled one with the hypotheses formed on the
# device and on the host
FORMS = ((None, False), ("cull", False), ("cull", True), ("mfma2", False), ("valu", False))
SWEEPS = (None, "cull", "mfma2", "valu")
SELECT_CLOUDS = ["lattice3d", "wide_lattice", "same", *E.FLAT] + [f"tiny{n}" for n in E.TINY_N]


def _form(monkeypatch, upper, host):
    for key, val in (("O3DX_RANSAC_UPPER", upper), ("O3DX_RANSAC_HOST_SETUP", "1" if host else None)):
        if val is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, val)


_DEV = {}


def _t(a, dev):
    """The array on the device (a copy: the catalogue's arrays are read-only), once per array."""
    if id(a) not in _DEV:
        _DEV[id(a)] = (torch.from_numpy(np.array(a, order="C")).to(dev), a)
    return _DEV[id(a)][0]


def _segment(c, x):
    plane, inl = ops.segment_plane(x, c.thr, c.rn, c.H, c.prob, samples=c.samples)
    return np.asarray(plane, np.float64), inl.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("cloud", F32)
def test_segment_plane_f32_every_form(dev, monkeypatch, cloud):
    """Every case of a float32 cloud under every sweep: the result against the
    reference by its class, and every form the same bits."""
    for cid in PC.ids(cloud=cloud):
        c = PC.cases()[cid]
        x = _t(c.pts, dev)
        first = None
        for upper, host in FORMS:
            _form(monkeypatch, upper, host)
            plane, inl = _segment(c, x)
            if first is None:
                PC.check_result(cid, plane, inl)
                first = (plane, inl)
            else:
                assert plane.tobytes() == first[0].tobytes() and np.array_equal(inl, first[1]), (cid, upper, host)
    _form(monkeypatch, None, False)


@pytest.mark.parametrize("cloud", F64)
def test_segment_plane_f64(dev, cloud):
    """The wide_ clouds through o3dx_segment_plane_f64, as tensors and through PointCloud."""
    pc = o3p.PointCloud(np.array(E.cloud(cloud)))
    assert pc._wide
    for cid in PC.ids(cloud=cloud):
        c = PC.cases()[cid]
        plane, inl = _segment(c, _t(c.pts, dev))
        PC.check_result(cid, plane, inl)
        p2, i2 = pc.segment_plane(c.thr, c.rn, c.H, c.prob, samples=c.samples)
        assert np.asarray(p2, np.float64).tobytes() == plane.tobytes(), cid
        assert np.array_equal(np.asarray(i2, np.int64), inl), cid


@pytest.mark.parametrize("cloud", F32 + F64)
def test_plane_count_exact_and_upper(dev, monkeypatch, cloud):
    """plane_count of every hypothesis of every case equals the plain count
    (-1 exactly at the degenerate ones); on float32 clouds every sweep's
    plane_count_upper is an upper bound with the same -1s, and plane_abs_sum
    on the tie sets is the reference's Sigma|d|."""
    bad = []
    for cid in PC.ids(cloud=cloud):
        c = PC.cases()[cid]
        if c.H == 0:
            continue
        r = PC.reference(cid)
        x = _t(c.pts, dev)
        got = ops.plane_count(x, r.planes, c.thr)
        assert np.array_equal(got, r.counts), (cid, np.nonzero(got != r.counts)[0][:8])
        if c.wide:
            continue
        for upper in SWEEPS:
            _form(monkeypatch, upper, False)
            ub = ops.plane_count_upper(x, r.planes, c.thr)
            assert np.array_equal(ub < 0, r.counts < 0) and (ub >= r.counts).all(), (cid, upper)
            assert (ub[r.counts < 0] == -1).all(), (cid, upper)
        _form(monkeypatch, None, False)
        if len(r.tied):
            s = ops.plane_abs_sum(x, r.planes, r.tied, c.thr)
            ref = r.sums[r.tied]
            err = np.abs(s - ref) / np.where(ref != 0, np.abs(ref), 1.0)
            print(f"{cid}: Sigma|d| over {len(r.tied)} tied, largest relative error {err.max():.3e} "
                  f"(reference sum there {ref[err.argmax()]:.3e})")
            if not np.allclose(s, ref, rtol=1e-12, atol=0):
                bad.append((cid, float(err.max()), float(ref[err.argmax()])))
        if cloud in E.FLAT and c.rn == 3:  # every hypothesis is the cloud's own plane
            which = np.nonzero(r.counts >= 0)[0].astype(np.int32)
            assert not ops.plane_abs_sum(x, r.planes, which, c.thr).any(), cid
    assert not bad, bad


def _select_planes(cloud):
    """(planes, thickness unit): the lattice plane z = 5 (normalised and not) and an oblique one."""
    if cloud == "wide_lattice":
        z = E.OFFSET[2] + 5 * 2.0 ** -4
        return [[0.0, 0.0, 1.0, -z], [0.0, 0.0, 2.0, -2 * z], [0.3, -1.2, 2.0, 5393380.0]], 2.0 ** -4
    return [[0.0, 0.0, 1.0, -5.0], [0.0, 0.0, 2.0, -10.0], [0.3, -1.2, 2.0, 0.1]], 1.0


def _thicknesses(s, unit):
    """Thickness exactly at a point's distance (strict: that point is out), its
    float64 neighbours, the open bands ending exactly at a layer and just past
    it, an empty band, everything."""
    a = np.sort(np.abs(s))
    t0 = float(a[len(a) // 2])
    up = float(np.nextafter(unit, 2 * unit))
    out = [unit, float(np.nextafter(unit, 0.0)), up, (-unit, unit), (-unit, up), (0.3, -0.3), 1e30, (-1e30, 1e30)]
    if t0 > 0:
        out += [t0, float(np.nextafter(t0, 0.0)), float(np.nextafter(t0, np.inf))]
    return out


@pytest.mark.parametrize("cloud", SELECT_CLOUDS)
def test_plane_select_and_distance_at_exact_thickness(dev, cloud):
    """plane_distance / plane_select (and distance2plane / get_index_by_plane
    through PointCloud) equal numpy on the reference's own expression,
    ((p * abc).sum(1) + d) / |abc|, bit for bit: thickness exactly at a point's
    distance, its neighbours, bands, the empty and the whole selection, invert."""
    pts = E.cloud(cloud)
    p64 = np.asarray(pts, np.float64)
    x = _t(pts, dev)
    pc = o3p.PointCloud(np.array(p64))
    assert pc._wide == cloud.startswith("wide_")
    planes, unit = _select_planes(cloud)
    sizes = set()
    for plane in planes:
        a, b, c, d = plane
        s = ((p64 * np.asarray([a, b, c])).sum(1) + d) / (a ** 2 + b ** 2 + c ** 2) ** 0.5
        got = ops.plane_distance(x, plane).cpu().numpy()
        assert got.dtype == np.float64 and np.array_equal(got, s), cloud
        assert np.array_equal(pc.distance2plane(plane), s)
        for thk in _thicknesses(s, unit):
            exp = np.logical_and(s > thk[0], s < thk[1]) if isinstance(thk, tuple) else np.abs(s) < thk
            sizes.add(int(exp.sum()))
            for inv in (False, True):
                want = np.nonzero(exp != inv)[0]
                assert np.array_equal(ops.plane_select(x, plane, thk, inv).cpu().numpy(), want), (cloud, plane, thk, inv)
                assert np.array_equal(pc.get_index_by_plane(plane, thk, invert=inv), want), (cloud, plane, thk, inv)
    assert 0 in sizes and len(pts) in sizes
    if cloud in ("lattice3d", "wide_lattice"):  # |s| < one layer step: the plane's own layer; the band past it adds one
        assert {144, 288}.issubset(sizes)


@pytest.mark.parametrize("cloud", [c for c in SELECT_CLOUDS if not c.startswith("wide_")])
def test_plane_inliers_at_exact_threshold(dev, cloud):
    """plane_inliers equals Open3D's predicate |(a x + c z) + (b y + d)| < thr
    at a threshold exactly at a point's distance and at its neighbours."""
    pts = E.cloud(cloud)
    x = _t(pts, dev)
    sizes = set()
    for plane in _select_planes(cloud)[0]:
        d = PC.open3d_dist(pts, plane)[:, 0]
        t0 = float(np.sort(d)[len(d) // 2])
        for thr in (1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0), 2.0, t0, np.nextafter(t0, 0.0),
                    np.nextafter(t0, np.inf), 1e30, 5e-324):
            want = np.nonzero(d < thr)[0]
            sizes.add(len(want))
            assert np.array_equal(ops.plane_inliers(x, plane, float(thr)).cpu().numpy(), want), (cloud, plane, thr)
    assert len(pts) in sizes
    if cloud == "lattice3d":
        assert {144, 432}.issubset(sizes)


def _seeds(seed0):
    seed = seed0
    while True:
        yield seed & 0xFFFFFFFF
        seed = (seed * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF


@pytest.mark.parametrize("cloud", ["line_x", "same"])
def test_seg_planes_ends_on_an_all_degenerate_cloud(cloud):
    """Every hypothesis of every round is degenerate: no plane, and the cloud
    comes back as the remainder.  (top_n = 5: a loop that does not end on the
    empty round returns six zero planes instead of spinning.)"""
    pts = np.asarray(E.cloud(cloud), np.float64)
    pc = o3p.PointCloud(np.array(pts))
    o3p.set_random_seed(11)
    planes, pcds, aabbs = pc.seg_planes(0.01, 3, 64, top_n=5)
    assert planes == [] and len(pcds) == 1 and len(aabbs) == 1
    assert np.array_equal(pcds[0].get_points(), pts)
    np.testing.assert_array_equal(aabbs[0][0], pts.min(0))
    np.testing.assert_array_equal(aabbs[0][1], pts.max(0))


def test_seg_planes_floor_and_cable_rounds_vs_oracle():
    """A floor (flatz@0) and a cable (line_x lifted by 0.5): round by round the
    oracle's SegmentPlane on the remaining points with the same seeded
    samples; the floor is the one plane, the round on the cable finds nothing
    and ends the loop, the cable is the remainder."""
    line = np.array(E.cloud("line_x"))
    line[:, 2] = 0.5
    pts = np.concatenate([E.cloud("flatz@0"), line]).astype(np.float32)
    n = len(pts)
    pc = o3p.PointCloud(pts.astype(np.float64))
    seed0, iters, thr, ratio = 11, 64, 0.01, 0.05
    o3p.set_random_seed(seed0)
    planes, pcds, aabbs = pc.seg_planes(thr, 3, iters, top_n=5, minPointsRatio=ratio)
    rest, r, seeds = np.arange(n), 0, _seeds(seed0)
    while len(rest) / n > ratio:
        samples = O.ransac_samples(len(rest), 3, iters, next(seeds))
        rplane, rinl, *_ = O.segment_plane(pts[rest], thr, 3, iters, samples)
        if len(rinl) == 0:
            break
        np.testing.assert_allclose(planes[r], rplane, atol=1e-9)
        sel = rest[rinl]
        assert np.array_equal(pcds[r].get_points(), pts[sel].astype(np.float64))
        np.testing.assert_array_equal(aabbs[r][0], pts[sel].min(0).astype(np.float64))
        np.testing.assert_array_equal(aabbs[r][1], pts[sel].max(0).astype(np.float64))
        rest = np.delete(rest, rinl)
        r += 1
        assert r <= 5
    assert r == 1 and len(planes) == 1 and len(pcds) == 2
    assert np.array_equal(np.abs(planes[0]), [0, 0, 1, 0])
    assert np.array_equal(pcds[0].get_points(), pts[:2000].astype(np.float64))
    assert np.array_equal(pcds[1].get_points(), line.astype(np.float64))


def test_seg_planes_one_round_takes_everything():
    pts = np.asarray(E.cloud("flat_nested"), np.float64)
    pc = o3p.PointCloud(np.array(pts))
    o3p.set_random_seed(11)
    planes, pcds, aabbs = pc.seg_planes(0.01, 3, 64, top_n=5)
    assert len(planes) == 1 and np.array_equal(np.abs(planes[0]), [0, 0, 1, 0.25])
    assert len(pcds) == 2 and np.array_equal(pcds[0].get_points(), pts) and pcds[1].size() == 0


@pytest.mark.parametrize("cid", ["flat_nested-n3-H300-t0.01", "flat_nested-n6-H300-t0.05", "lattice3d-n3-H300-t1"])
def test_reruns_are_bit_identical(dev, cid):
    """A case whose hypotheses tie (every one holds the whole flat cloud;
    lattice planes with equal counts): the same bits on every run."""
    c = PC.cases()[cid]
    assert len(PC.reference(cid).tied) >= 2 or PC.reference(cid).counts.max() == len(c.pts)
    x = _t(c.pts, dev)
    first = _segment(c, x)
    PC.check_result(cid, *first)
    for _ in range(3):
        plane, inl = _segment(c, x)
        assert plane.tobytes() == first[0].tobytes() and np.array_equal(inl, first[1])
