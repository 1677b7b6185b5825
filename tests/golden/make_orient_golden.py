"""Writes tests/golden/orient_ref.npz: the normal-orientation cases and the
answers of the numpy restatement (tests/orient_oracle.py).

    python tests/golden/make_orient_golden.py

Needs scipy (cross-checks only); the tests read only the file.  Per case: the
float32 points, the float32 normals fed in (stored, not recomputed: equal signs
need bit-identical inputs), the ks, the EMST edges, and per k the tree edges
and the flip bytes (packed bits).

Asserted here for every case, and stored (<case>_checks = {tie-invariant,
scipy weight compared, Delaunay compared}):
  - the flips are the same under ascending and descending tie order;
  - without zero distances, the EMST's total weight equals
    scipy.sparse.csgraph.minimum_spanning_tree's on the dense matrix (scipy
    drops zero weights, so clouds with duplicate points are exempt);
  - for the non-degenerate clouds every EMST edge is an edge of
    scipy.spatial.Delaunay(points), the route Open3D takes to the same tree.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "open3d-py-extension_amd"))
import orient_oracle as OO  # noqa: E402

OUT = os.path.join(HERE, "orient_ref.npz")


def shell(rng, n, centre, radius, noise=0.01):
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    r = radius * (1.0 + noise * rng.standard_normal((n, 1)))
    return np.asarray(centre, np.float64) + r * v


def bunny_points():
    from open3dpypro.pcd_io import read_pcd_arrays
    from oracle.np_restate import voxel_down_sample

    f = read_pcd_arrays(os.path.join(HERE, "bunny.pcd"))
    p = np.stack([f["x"], f["y"], f["z"]], 1).astype(np.float32)
    return p[voxel_down_sample(p, 0.005)]


def cases():
    """name, float32 points, float32 normals, ks, compare scipy weight, compare Delaunay"""
    rng = np.random.default_rng(20240917)
    p = shell(rng, 1500, (0, 0, 0), 1.0).astype(np.float32)
    yield "sphere", p, OO.pca_normals(p, 10), (10,), True, True
    p = np.concatenate([shell(rng, 300, (0, 0, 0), 0.5), shell(rng, 300, (2, 0, 0), 0.5)])
    p = p[rng.permutation(len(p))].astype(np.float32)
    yield "blobs", p, OO.pca_normals(p, 8), (8,), True, True
    centres = [(0, 0, 0), (1.5, 0.2, 0.1), (0.3, 1.7, -0.2), (-1.2, -0.9, 0.8), (0.6, 0.5, 2.4)]
    parts = [shell(rng, m, c, r) for m, c, r in zip((40, 70, 100, 25, 160), centres, (0.3, 0.4, 0.5, 0.2, 0.6))]
    p = np.concatenate(parts).astype(np.float32)
    p = np.concatenate([p, p[rng.choice(len(p), 7, replace=False)]])
    p = p[rng.permutation(len(p))]
    assert len(p) == 402
    yield "clusters", p, OO.pca_normals(p, 6), (3, 6), False, False
    g = np.stack(np.meshgrid(np.arange(32), np.arange(32), indexing="ij"), -1).reshape(-1, 2) * 0.125
    p = np.concatenate([g, np.zeros((len(g), 1))], 1).astype(np.float32)
    nrm = np.zeros((len(p), 3), np.float32)
    nrm[:, 2] = rng.choice([-1.0, 1.0], len(p))
    yield "lattice", p, nrm, (5, 9), True, False
    p = bunny_points()
    yield "bunny", p, OO.pca_normals(p, 30), (30,), True, True


def main():
    from scipy.sparse.csgraph import minimum_spanning_tree
    from scipy.spatial import Delaunay

    out = {}
    names = []
    for name, p, nrm, ks, scipy_weight, delaunay in cases():
        n = len(p)
        d2 = OO.d2_dense(p)
        E = OO.emst(p, d2)
        Er = OO.emst(p, d2, reverse_ties=True)
        w = float(d2[E[:, 0], E[:, 1]].sum())
        assert np.isclose(w, float(d2[Er[:, 0], Er[:, 1]].sum()), rtol=1e-12), name
        if scipy_weight:
            assert (d2[np.triu_indices(n, 1)] > 0).all(), name
            ws = float(minimum_spanning_tree(d2).sum())
            assert np.isclose(w, ws, rtol=1e-12), (name, w, ws)
        if delaunay:
            tri = Delaunay(p.astype(np.float64)).simplices
            de = set()
            for a in range(4):
                for b in range(a + 1, 4):
                    lo, hi = np.minimum(tri[:, a], tri[:, b]), np.maximum(tri[:, a], tri[:, b])
                    de.update(zip(lo.tolist(), hi.tolist()))
            assert all(tuple(e) in de for e in E.tolist()), name
        out.update({f"{name}_pts": p, f"{name}_normals": nrm, f"{name}_ks": np.asarray(ks, np.int32),
                    f"{name}_emst": E, f"{name}_checks": np.asarray([1, int(scipy_weight), int(delaunay)], np.int8)})
        for k in ks:
            r = OO.orient(p, nrm, k, d2=d2, emst_edges=E)
            rr = OO.orient(p, nrm, k, reverse_ties=True, d2=d2, emst_edges=Er)
            assert np.array_equal(r["flip"], rr["flip"]), (name, k)
            out[f"{name}_tree{k}"] = r["tree"]
            out[f"{name}_flip{k}"] = np.packbits(r["flip"])
            print(f"{name}: n={n} k={k} EMST edges outside the kNN graph={r['outside']} flipped={int(r['flip'].sum())} "
                  f"root={OO.root_index(p)}")
            if name == "sphere":
                assert ((r["normals"].astype(np.float64) * p).sum(1) > 0).all()
            if name == "lattice":
                assert np.array_equal(r["normals"], np.tile(np.float32([0, 0, 1]), (n, 1)))
        names.append(name)
    out["cases"] = np.asarray(names)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 1 << 20


if __name__ == "__main__":
    main()
