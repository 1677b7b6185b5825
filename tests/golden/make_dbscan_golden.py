"""Writes tests/golden/dbscan_ref.npz: the DBSCAN cases and sklearn's answers.

    python tests/golden/make_dbscan_golden.py

Needs scikit-learn (the reference's clustering: sklearn.cluster.DBSCAN behind
PointCloud.DBSCAN); the tests read only the file.  Per case: points (float32,
or float64 for the wide case; the scale case's come from
tests/test_dbscan.py hash_points and are not stored), eps, min_samples,
sklearn's labels_ (int32) and its core mask (packed bits).

Condition on the inputs (asserted here): no pair of points at a distance
within eps (1 +- 1e-7) — sklearn's KD-tree may accept a whole node by a bound,
so a pair that close to eps is not pinned by it.  The lattice is exempt: its
coordinates and sums are exact integers.  The scale case's eps is the first
value from 0.02 upwards (steps of 1e-5) that meets the condition.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "open3d-py-extension_amd"))
from test_dbscan import d2_exact, hash_points, pairs_dense, pairs_grid  # noqa: E402

OUT = os.path.join(HERE, "dbscan_ref.npz")


def band_pairs(p, eps):
    p = np.asarray(p, np.float64)
    i, j = (pairs_dense if len(p) <= 5000 else pairs_grid)(p, eps * (1 + 2e-7))
    d = np.sqrt(d2_exact(p[i], p[j]))
    return int(((d >= eps * (1 - 1e-7)) & (d <= eps * (1 + 1e-7))).sum())


def blobs(rng, n_blob, n_clutter, centres, sigma=0.05):
    parts = [c + sigma * rng.standard_normal((n_blob, 3)) for c in centres]
    parts.append(rng.random((n_clutter, 3)))
    p = np.concatenate(parts)
    return p[rng.permutation(len(p))]


def cases():
    rng = np.random.default_rng(20240611)
    centres = np.array([[0.25, 0.25, 0.3], [0.75, 0.3, 0.6], [0.3, 0.75, 0.7], [0.7, 0.75, 0.25]])
    yield "uniform", rng.random((4000, 3)).astype(np.float32), 0.06, 5
    yield "blobs", blobs(rng, 700, 400, centres).astype(np.float32), 0.04, 6
    lat = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(3), indexing="ij"), -1).reshape(-1, 3)
    yield "lattice", lat[rng.permutation(len(lat))[:400]].astype(np.float32), 1.0, 4
    d = np.repeat(rng.random((300, 3)).astype(np.float32), 3, axis=0)
    yield "dups", d[rng.permutation(900)], 0.05, 4
    chain = np.zeros((3000, 3), np.float32)
    chain[:, 0] = (np.arange(3000) * 0.01).astype(np.float32)
    yield "chain", chain[rng.permutation(3000)], 0.0125, 3
    wide = blobs(rng, 525, 400, centres) + np.array([5e5, 4.2e6, 300.0])
    assert not np.array_equal(wide.astype(np.float32).astype(np.float64), wide)
    yield "wide", wide, 0.04, 6


def main():
    from sklearn.cluster import DBSCAN

    def fit(p, eps, ms):
        m = DBSCAN(eps=eps, min_samples=ms).fit(np.asarray(p, np.float64))
        core = np.zeros(len(p), bool)
        core[m.core_sample_indices_] = True
        return m.labels_.astype(np.int32), core

    out = {}
    for name, p, eps, ms in cases():
        if name != "lattice":
            assert band_pairs(p, eps) == 0, name
        labels, core = fit(p, eps, ms)
        out.update({f"{name}_pts": p, f"{name}_n": len(p), f"{name}_eps": eps, f"{name}_ms": ms,
                    f"{name}_labels": labels, f"{name}_core": np.packbits(core)})
        print(f"{name}: n={len(p)} clusters={labels.max() + 1} core={core.sum()} noise={(labels < 0).sum()}")
        if name == "wide":
            l32, _ = fit(p.astype(np.float32), eps, ms)
            assert not np.array_equal(l32, labels)
            out["wide_labels_f32"] = l32
    n = 100000
    p = hash_points(n)
    eps = 0.02
    while band_pairs(p, eps):
        eps = round(eps + 1e-5, 5)
    labels, core = fit(p, eps, 5)
    out.update(scale_n=n, scale_eps=eps, scale_ms=5, scale_labels=labels, scale_core=np.packbits(core))
    print(f"scale: n={n} eps={eps} clusters={labels.max() + 1} core={core.sum()} noise={(labels < 0).sum()}")
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")
    assert os.path.getsize(OUT) < 1 << 20


if __name__ == "__main__":
    main()
