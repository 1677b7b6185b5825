"""DBSCAN on the GPU against sklearn's stored answers (tests/golden/dbscan_ref.npz)
and the numpy restatement of the rule (test_dbscan.py).  Labels are compared
with array_equal: the fixture's inputs have no pair within rounding of eps."""
import numpy as np
import pytest
import torch

import open3dpypro as o3p
from open3dpypro import ops
from test_dbscan import CASES, case, dbscan_restate, n_clusters, pairs_dense

pytestmark = pytest.mark.gpu


def run(pts, eps, ms, dev):
    labels, k, core = ops.dbscan(torch.as_tensor(np.array(pts), device=dev), eps, ms, return_core=True)
    assert labels.dtype == torch.int32 and core.dtype == torch.bool and labels.device.type == "cuda"
    return labels.cpu().numpy(), k, core.cpu().numpy()


@pytest.mark.parametrize("name", CASES)
def test_fixture_cases(name, dev):
    c = case(name)
    labels, k, core = run(c["pts"], c["eps"], c["min_samples"], dev)
    assert np.array_equal(core, c["core"])
    assert np.array_equal(labels, c["labels"])
    assert k == n_clusters(c["labels"])


def test_wide_cloud_through_pointcloud_takes_the_float64_entry(dev):
    c = case("wide")
    pc = o3p.PointCloud(np.array(c["pts"]))
    assert pc._wide and pc._hot_points().dtype == torch.float64
    pcds, labels = pc.DBSCAN(c["eps"], c["min_samples"])
    assert labels.dtype == np.int64 and np.array_equal(labels, c["labels"])
    assert not np.array_equal(labels, c["labels_f32"])
    assert len(pcds) == n_clusters(c["labels"])
    for i, q in enumerate(pcds):
        assert np.array_equal(q.get_points(), c["pts"][c["labels"] == i])
    # the same values narrowed to float32: the float32 entry, sklearn's labels of those points
    l32, _, _ = run(c["pts"].astype(np.float32), c["eps"], c["min_samples"], dev)
    assert np.array_equal(l32, c["labels_f32"])


@pytest.fixture(scope="module")
def uniform_pairs():
    """The uniform case's pair lists per eps of the sweep, computed once."""
    p = case("uniform")["pts"]
    return {eps: pairs_dense(p, eps) for eps in (1e-4, 0.06, 2.0)}


@pytest.mark.parametrize("eps", [1e-4, 0.06, 2.0])
@pytest.mark.parametrize("ms", [1, 2, 30])
def test_sweep_against_the_restatement(eps, ms, dev, uniform_pairs):
    p = case("uniform")["pts"]
    want, wcore = dbscan_restate(p, eps, ms, pairs=uniform_pairs[eps])
    labels, k, core = run(p, eps, ms, dev)
    assert np.array_equal(core, wcore) and np.array_equal(labels, want) and k == n_clusters(want)
    if eps == 1e-4:  # no two points that close: singletons numbered by index, or all noise
        assert np.array_equal(labels, np.arange(4000) if ms == 1 else np.full(4000, -1))
    if eps == 2.0:  # the whole cube: one cluster from a one-cell grid
        assert (labels == 0).all() and k == 1


def test_single_point(dev):
    p = np.array([[0.3, -1.0, 7.0]], np.float32)
    for ms, want in ((1, 0), (2, -1)):
        labels, k, core = run(p, 0.5, ms, dev)
        assert labels.tolist() == [want] and k == want + 1 and core.tolist() == [want == 0]
        labels, k, core = run(p.astype(np.float64) + 1e-9, 0.5, ms, dev)
        assert labels.tolist() == [want] and k == want + 1 and core.tolist() == [want == 0]


def test_large_coordinates_against_eps(dev):
    """float32 points far from the origin against eps: the cell-assignment
    slack exceeds the first grid's margin, so the grid is rebuilt wider."""
    c = case("blobs")
    p = (c["pts"] + np.float32(4096.0)).astype(np.float32)
    want, wcore = dbscan_restate(p, c["eps"], c["min_samples"])
    labels, k, core = run(p, c["eps"], c["min_samples"], dev)
    assert np.array_equal(core, wcore) and np.array_equal(labels, want) and k == n_clusters(want)


def test_deterministic_and_order_follows_smallest_core_index(dev):
    c = case("uniform")
    a = run(c["pts"], c["eps"], c["min_samples"], dev)
    b = run(c["pts"], c["eps"], c["min_samples"], dev)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and a[1] == b[1]
    perm = np.random.default_rng(5).permutation(len(c["pts"]))
    q = c["pts"][perm]
    want, wcore = dbscan_restate(q, c["eps"], c["min_samples"])
    labels, k, core = run(q, c["eps"], c["min_samples"], dev)
    assert np.array_equal(core, wcore) and np.array_equal(labels, want)
    assert not np.array_equal(labels, a[0][perm])  # renumbered, not carried over
    # the same partition of the core points either way (a border point between
    # two clusters follows the numbering)
    assert np.array_equal(core, a[2][perm])
    m = {}
    for x, y in zip(labels[core].tolist(), a[0][perm][core].tolist()):
        assert m.setdefault(x, y) == y
    assert len(set(m.values())) == len(m) == k


def test_pointcloud_dbscan_carries_every_attribute(dev):
    c = case("blobs")
    rng = np.random.default_rng(9)
    n = len(c["pts"])
    rgb, nrm = rng.random((n, 3)).astype(np.float32), rng.standard_normal((n, 3)).astype(np.float32)
    inten = rng.random((n, 1))
    pc = o3p.PointCloud(np.array(c["pts"]), rgb=rgb, normals=nrm, intensity=inten)
    pcds, labels = pc.DBSCAN(c["eps"], c["min_samples"])
    assert isinstance(labels, np.ndarray) and labels.dtype == np.int64 and np.array_equal(labels, c["labels"])
    assert len(pcds) == n_clusters(c["labels"]) == 4
    for i, q in enumerate(pcds):
        sel = labels == i
        assert isinstance(q, o3p.PointCloud) and q.size() == sel.sum()
        assert np.array_equal(q.get_points(), c["pts"][sel].astype(np.float64))
        assert np.array_equal(q.get_colors().astype(np.float32), rgb[sel])
        assert np.array_equal(q.get_normals().astype(np.float32), nrm[sel])
        assert np.array_equal(q.get_intensity(), inten[sel])
    # the reference's defaults
    pcds, labels = o3p.PointCloud(np.array(case("dups")["pts"])).DBSCAN()
    want, _ = dbscan_restate(case("dups")["pts"], 0.05, 3)
    assert np.array_equal(labels, want) and len(pcds) == n_clusters(want)
