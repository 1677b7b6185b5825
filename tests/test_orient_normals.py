"""Normal orientation, host side: the numpy restatement (orient_oracle.py)
re-checked on the committed fixture (tests/golden/orient_ref.npz, written by
tests/golden/make_orient_golden.py), the argument checks that run before any
GPU work, the two torch-only sibling methods and the ABI table."""
import os

import numpy as np
import pytest
import torch

import open3dpypro as o3p
import orient_oracle as OO
from conftest import GOLDEN
from open3dpypro import _native as N

_REF = None
CASES = ["sphere", "blobs", "clusters", "lattice", "bunny"]


def ref():
    global _REF
    if _REF is None:
        with np.load(os.path.join(GOLDEN, "orient_ref.npz")) as z:
            _REF = {k: z[k] for k in z.files}
    return _REF


def case(name):
    r = ref()
    pts = r[f"{name}_pts"]
    ks = [int(k) for k in r[f"{name}_ks"]]
    return {"pts": pts, "normals": r[f"{name}_normals"], "ks": ks, "emst": r[f"{name}_emst"],
            "checks": r[f"{name}_checks"].tolist(),
            "tree": {k: r[f"{name}_tree{k}"] for k in ks},
            "flip": {k: np.unpackbits(r[f"{name}_flip{k}"])[:len(pts)].astype(bool) for k in ks}}


def oriented(c, k):
    out = c["normals"].copy()
    out[c["flip"][k]] = -out[c["flip"][k]]
    return out


def test_fixture_lists_the_cases():
    assert ref()["cases"].tolist() == CASES
    sizes = {n: len(case(n)["pts"]) for n in CASES}
    assert sizes == {"sphere": 1500, "blobs": 600, "clusters": 402, "lattice": 1024, "bunny": 3017}
    for n in CASES:
        c = case(n)
        assert c["pts"].dtype == np.float32 and c["normals"].dtype == np.float32
        assert c["emst"].shape == (sizes[n] - 1, 2) and (c["emst"][:, 0] < c["emst"][:, 1]).all()


@pytest.mark.parametrize("name", CASES)
def test_oracle_self_checks_on_the_fixture(name):
    from scipy.sparse.csgraph import minimum_spanning_tree
    from scipy.spatial import Delaunay

    c = case(name)
    p, n = c["pts"], len(c["pts"])
    d2 = OO.d2_dense(p)
    E = OO.emst(p, d2)
    assert np.array_equal(E, c["emst"])
    Er = OO.emst(p, d2, reverse_ties=True)
    tie_inv, scipy_weight, delaunay = c["checks"]
    assert tie_inv == 1
    w = float(d2[E[:, 0], E[:, 1]].sum())
    if scipy_weight:
        assert (d2[np.triu_indices(n, 1)] > 0).all()
        assert np.isclose(w, float(minimum_spanning_tree(d2).sum()), rtol=1e-12)
    if delaunay:
        tri = Delaunay(p.astype(np.float64)).simplices
        de = set()
        for a in range(4):
            for b in range(a + 1, 4):
                lo, hi = np.minimum(tri[:, a], tri[:, b]), np.maximum(tri[:, a], tri[:, b])
                de.update(zip(lo.tolist(), hi.tolist()))
        assert all(tuple(e) in de for e in E.tolist())
    for k in c["ks"]:
        r = OO.orient(p, c["normals"], k, d2=d2, emst_edges=E)
        assert np.array_equal(r["tree"], c["tree"][k]) and np.array_equal(r["flip"], c["flip"][k])
        rr = OO.orient(p, c["normals"], k, reverse_ties=True, d2=d2, emst_edges=Er)
        assert np.array_equal(rr["flip"], r["flip"])  # the fixture does not hinge on a tie
        assert np.array_equal(np.abs(r["normals"]), np.abs(c["normals"]))


def test_fixture_properties():
    c = case("sphere")
    assert ((oriented(c, 10).astype(np.float64) * c["pts"]).sum(1) > 0).all()  # every normal outward
    c = case("lattice")
    for k in c["ks"]:
        assert np.array_equal(oriented(c, k), np.tile(np.float32([0, 0, 1]), (1024, 1)))
    c = case("blobs")  # the kNN graph is disconnected: one EMST edge joins the shells
    r = OO.orient(c["pts"], c["normals"], 8, emst_edges=c["emst"])
    assert r["outside"] == 1
    c = case("clusters")
    assert OO.orient(c["pts"], c["normals"], 3, emst_edges=c["emst"])["outside"] > 20
    d2 = OO.d2_dense(c["pts"])
    assert (d2[np.triu_indices(402, 1)] == 0).sum() >= 7  # duplicated points: zero weights


def test_oracle_edge_cases():
    one = np.float32([[0.1, 0.2, 0.3]])
    for nz, want in ((-1.0, True), (1.0, False), (-0.0, False)):
        r = OO.orient(one, np.float32([[0, 0, nz]]), 5)
        assert r["flip"].tolist() == [want] and r["tree"].shape == (0, 2)
    two = np.float32([[0, 0, 0], [1, 0, 0]])  # equal z: the lower index roots
    r = OO.orient(two, np.float32([[0, 0, -1], [0, 0, 1]]), 30)
    assert r["flip"].tolist() == [True, False] and r["tree"].tolist() == [[0, 1]]
    r = OO.orient(two[::-1], np.float32([[0, 0, 1], [0, 0, -1]]), 1)
    assert r["flip"].tolist() == [False, True]
    r = OO.orient(two, np.float32([[0, 0, 1], [1, 0, 0]]), 2)  # dot == 0 never flips
    assert r["flip"].tolist() == [False, False]


def test_poisson_without_normals_raises_runtime_error():
    pc = o3p.PointCloud(np.random.default_rng(0).random((8, 3)).astype(np.float32))
    with pytest.raises(RuntimeError):
        pc.estimate_normals(method="poisson")
    with pytest.raises(RuntimeError):
        pc.orient_normals_consistent_tangent_plane()
    for f in (pc.orient_normals_to_align_with_direction, pc.orient_normals_towards_camera_location):
        with pytest.raises(RuntimeError):
            f()


def test_bad_k_raises_value_error():
    p = np.random.default_rng(1).random((8, 3)).astype(np.float32)
    pc = o3p.PointCloud(p, normals=np.tile(np.float32([0, 0, 1]), (8, 1)))
    for k in (0, -3, 2.5):
        with pytest.raises(ValueError):
            pc.orient_normals_consistent_tangent_plane(k=k)


def test_empty_cloud_is_left_alone_and_non_finite_points_are_rejected():
    pc = o3p.PointCloud()
    assert pc.orient_normals_consistent_tangent_plane() is pc and pc.estimate_normals(method="poisson") is pc
    p = np.random.default_rng(2).random((8, 3)).astype(np.float32)
    p[3, 1] = np.nan
    pc = o3p.PointCloud(torch.as_tensor(p), normals=np.tile(np.float32([0, 0, 1]), (8, 1)))
    with pytest.raises(ValueError):
        pc.orient_normals_consistent_tangent_plane()


def test_wide_cloud_raises_not_implemented_before_any_gpu_work():
    p = np.random.default_rng(3).random((8, 3)) + 4.2e6
    pc = o3p.PointCloud(p, normals=np.tile(np.float32([0, 0, 1]), (8, 1)))
    assert pc._wide
    with pytest.raises(NotImplementedError, match="float64"):
        pc.estimate_normals(method="poisson")


def test_align_with_direction():
    nrm = np.float32([[0, 0, 1], [0, 0, -2], [1, 0, 0], [0, 0, 0], [0.5, 0.5, -1e-3], [-0.0, 0.0, 0.0]])
    pc = o3p.PointCloud(torch.zeros((6, 3)), normals=torch.as_tensor(nrm))
    assert pc.orient_normals_to_align_with_direction() is pc
    want = np.float32([[0, 0, 1], [0, 0, 2], [1, 0, 0], [0, 0, 1], [-0.5, -0.5, 1e-3], [0, 0, 1]])
    assert np.array_equal(pc.get_normals().astype(np.float32), want)
    pc = o3p.PointCloud(torch.zeros((6, 3)), normals=torch.as_tensor(nrm))
    pc.orient_normals_to_align_with_direction((-1.0, 0.0, 0.0))
    want = np.float32([[0, 0, 1], [0, 0, -2], [-1, 0, 0], [-1, 0, 0], [-0.5, -0.5, 1e-3], [-1, 0, 0]])
    assert np.array_equal(pc.get_normals().astype(np.float32), want)


def test_towards_camera_location():
    pts = np.float32([[1, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 0], [3, 0, 4], [0, 1, 0]])
    nrm = np.float32([[1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, 0, 0], [0, 0, 0], [1, 0, 0]])
    pc = o3p.PointCloud(torch.as_tensor(pts), normals=torch.as_tensor(nrm))
    assert pc.orient_normals_towards_camera_location() is pc
    # ref = -point: towards the origin; dot == 0 keeps; zero normal -> ref normalised, (0,0,1) at the camera
    want = np.float32([[-1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, 0, 1], [-0.6, 0, -0.8], [1, 0, 0]])
    got = pc.get_normals().astype(np.float32)
    assert np.array_equal(got[[0, 1, 2, 3, 5]], want[[0, 1, 2, 3, 5]])
    assert np.allclose(got[4], want[4], rtol=0, atol=1e-7)
    pc = o3p.PointCloud(torch.as_tensor(pts), normals=torch.as_tensor(nrm))
    pc.orient_normals_towards_camera_location((10.0, 0.0, 0.0))
    assert np.array_equal(pc.get_normals().astype(np.float32)[:2], np.float32([[1, 0, 0], [1, 0, 0]]))


def test_abi_table_lists_the_new_entries():
    names = ["o3dx_emst_workspace_bytes", "o3dx_emst", "o3dx_orient_normals_workspace_bytes",
             "o3dx_orient_normals_tangent_plane"]
    syms = N.declared_symbols()
    with open(N.HEADER_PATH) as f:
        header = f.read()
    for s in names:
        assert s in syms and f"{s}(" in header
    assert "#define O3DX_ABI_VERSION 7" in header  # additive: the number stays
