"""EMST and consistent normal orientation on the GPU against the stored
answers of the numpy restatement (tests/golden/orient_ref.npz) and the
restatement itself (orient_oracle.py).  Every comparison is exact: the rule's
strict total order on edges leaves nothing to a tie."""
import numpy as np
import pytest
import torch

import open3dpypro as o3p
import orient_oracle as OO
from open3dpypro import ops
from test_orient_normals import CASES, case, oriented

pytestmark = pytest.mark.gpu

CASE_KS = [(n, k) for n in CASES for k in case(n)["ks"]]


def t(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def run(p, nrm, k, dev):
    out, tree, flip = ops.orient_normals_tangent_plane(t(p, dev), t(nrm, dev), k, return_tree=True)
    assert out.dtype == torch.float32 and tree.dtype == torch.int32 and flip.dtype == torch.bool
    assert out.device.type == "cuda" and tree.shape == (max(len(p) - 1, 0), 2)
    return out.cpu().numpy(), tree.cpu().numpy(), flip.cpu().numpy()


@pytest.mark.parametrize("name", CASES)
def test_emst_equals_the_fixture(name, dev):
    c = case(name)
    e = ops.emst(t(c["pts"], dev))
    assert e.dtype == torch.int32 and e.device.type == "cuda"
    assert np.array_equal(e.cpu().numpy(), c["emst"])


@pytest.mark.parametrize("name,k", CASE_KS)
def test_tree_and_flips_equal_the_fixture(name, k, dev):
    c = case(name)
    out, tree, flip = run(c["pts"], c["normals"], k, dev)
    assert np.array_equal(tree, c["tree"][k])
    assert np.array_equal(flip, c["flip"][k])
    assert np.array_equal(out.view(np.uint32) & 0x7fffffff, c["normals"].view(np.uint32) & 0x7fffffff)
    assert np.array_equal(out.view(np.uint32), oriented(c, k).view(np.uint32))


@pytest.mark.parametrize("name,k", CASE_KS)
def test_through_pointcloud(name, k, dev):
    c = case(name)
    pc = o3p.PointCloud(t(c["pts"], dev), normals=t(c["normals"], dev))
    if name == "bunny":
        assert k == 30 and pc.estimate_normals(method="poisson") is pc  # the API's own path
    else:
        assert pc.orient_normals_consistent_tangent_plane(k) is pc
    assert np.array_equal(pc.get_normals(), oriented(c, k).astype(np.float64))
    assert np.array_equal(pc.get_points(), c["pts"].astype(np.float64))  # nothing else changes


def test_sphere_normals_point_outward(dev):
    c = case("sphere")
    out, _, _ = run(c["pts"], c["normals"], 10, dev)
    assert ((out.astype(np.float64) * c["pts"]).sum(1) > 0).all()


@pytest.mark.parametrize("k", [5, 9])
def test_lattice_normals_all_up(k, dev):
    c = case("lattice")
    out, _, _ = run(c["pts"], c["normals"], k, dev)
    assert np.array_equal(out, np.tile(np.float32([0, 0, 1]), (1024, 1)))


def test_two_runs_are_bit_identical(dev):
    c = case("clusters")
    a = run(c["pts"], c["normals"], 3, dev)
    b = run(c["pts"], c["normals"], 3, dev)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert np.array_equal(ops.emst(t(c["pts"], dev)).cpu().numpy(), ops.emst(t(c["pts"], dev)).cpu().numpy())


def test_independent_of_the_input_order(dev):
    """A fixed permutation of the clusters case, results mapped back.  The
    max-z point is unique, so the root is the same point.  The flips are the
    same; so is the EMST's edge set once the 7 duplicated points are
    identified with their twins (between a point and two twins the two edges
    weigh the same, and the total order picks by index).  On the permuted
    input itself the result equals the restatement's exactly."""
    c = case("clusters")
    p, nrm = c["pts"], c["normals"]
    assert (p[:, 2] == p[:, 2].max()).sum() == 1
    perm = np.random.default_rng(7).permutation(len(p))
    _, twin = np.unique(p, axis=0, return_inverse=True)
    twin = twin.reshape(-1)

    def canon(e):
        a = np.sort(twin[e.astype(np.int64)], 1)
        return set(map(tuple, a[a[:, 0] != a[:, 1]].tolist()))

    e = ops.emst(t(p[perm], dev)).cpu().numpy()
    assert np.array_equal(e, OO.emst(p[perm]))
    assert canon(perm[e.astype(np.int64)]) == canon(c["emst"])
    for k in c["ks"]:
        _, tree, flip = run(p[perm], nrm[perm], k, dev)
        r = OO.orient(p[perm], nrm[perm], k)
        assert np.array_equal(tree, r["tree"]) and np.array_equal(flip, r["flip"])
        back = np.zeros(len(p), bool)
        back[perm] = flip
        assert np.array_equal(back, c["flip"][k])


def test_end_to_end_on_the_projects_own_normals(bunny, dev):
    pc = o3p.PointCloud(bunny).voxel_down_sample(0.005).estimate_normals()
    p = pc.get_points().astype(np.float32)
    nrm = pc.get_normals().astype(np.float32)  # the GPU's normals, before orienting
    assert len(p) == 3017
    assert pc.estimate_normals(method="poisson") is pc
    r = OO.orient(p, nrm, 30)
    assert np.array_equal(pc.get_normals().astype(np.float32).view(np.uint32), r["normals"].view(np.uint32))
    assert 0 < r["flip"].sum() < len(p)


def test_edge_cases(dev):
    one = np.float32([[0.1, 0.2, 0.3]])
    for nz, want in ((-1.0, True), (1.0, False), (-0.0, False)):  # n = 1: the root rule only
        out, tree, flip = run(one, np.float32([[0.5, 0, nz]]), 5, dev)
        assert flip.tolist() == [want] and tree.shape == (0, 2)
        assert np.array_equal(out, np.float32([[-0.5, -0.0, 1.0]]) if want else np.float32([[0.5, 0, nz]]))
    assert ops.emst(t(one, dev)).shape == (0, 2)
    two = np.float32([[0, 0, 0], [1, 0, 0]])  # n = 2, k > n, equal z: the lower index roots
    out, tree, flip = run(two, np.float32([[0, 0, -1], [0, 0, 1]]), 30, dev)
    assert flip.tolist() == [True, False] and tree.tolist() == [[0, 1]]
    assert np.array_equal(out, np.float32([[-0.0, -0.0, 1], [0, 0, 1]]))
    assert ops.emst(t(two, dev)).tolist() == [[0, 1]]
    _, _, flip = run(two[::-1], np.float32([[0, 0, 1], [0, 0, -1]]), 1, dev)
    assert flip.tolist() == [False, True]
    _, _, flip = run(two, np.float32([[0, 0, 1], [1, 0, 0]]), 2, dev)  # dot == 0 never flips
    assert flip.tolist() == [False, False]
    # fewer than 4 points, coplanar, collinear, duplicated: all work
    rng = np.random.default_rng(11)
    for p in (rng.random((3, 3)), np.c_[rng.random((9, 2)), np.zeros(9)], np.c_[np.arange(7.0), np.zeros((7, 2))],
              np.repeat(rng.random((2, 3)), 4, axis=0)):
        p = p.astype(np.float32)
        nrm = rng.standard_normal(p.shape).astype(np.float32)
        for k in (1, 2, 40):
            r = OO.orient(p, nrm, k)
            out, tree, flip = run(p, nrm, k, dev)
            assert np.array_equal(tree, r["tree"]) and np.array_equal(flip, r["flip"])
            assert np.array_equal(out.view(np.uint32), r["normals"].view(np.uint32))
        assert np.array_equal(ops.emst(t(p, dev)).cpu().numpy(), r["emst"])
    # empty cloud: a no-op
    out, tree, flip = run(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), 3, dev)
    assert out.shape == (0, 3) and tree.shape == (0, 2) and flip.shape == (0,)
    assert ops.emst(t(np.zeros((0, 3), np.float32), dev)).shape == (0, 2)


def test_bad_arguments(dev):
    c = case("blobs")
    with pytest.raises(ValueError):
        ops.orient_normals_tangent_plane(t(c["pts"], dev), t(c["normals"], dev), 0)
    wide = c["pts"].astype(np.float64) + 4.2e6 + 1e-9
    pc = o3p.PointCloud(wide, normals=c["normals"])
    assert pc._wide
    with pytest.raises(NotImplementedError, match="float64"):
        pc.orient_normals_consistent_tangent_plane(8)
    with pytest.raises(NotImplementedError, match="float64"):
        ops.emst(t(wide, dev))
