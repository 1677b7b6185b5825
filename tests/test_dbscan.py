"""DBSCAN (PointCloud.DBSCAN, ops.dbscan, o3dx_dbscan): the host side.

The rule (include/o3dx.h "clustering") is restated here in numpy and pinned
against the fixture tests/golden/dbscan_ref.npz, which holds sklearn's labels
and core masks (tests/golden/make_dbscan_golden.py writes it).  Nothing here
needs a GPU; the GPU tests (test_gpu_dbscan.py) import the restatement and the
scale case's generator from this file.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import open3dpypro as o3p
from open3dpypro import _native as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dbscan_ref.npz")
STORED = ("uniform", "blobs", "lattice", "dups", "chain", "wide")  # cases whose points are in the fixture
CASES = STORED + ("scale",)
SYMBOLS = ("o3dx_dbscan_workspace_bytes", "o3dx_dbscan", "o3dx_dbscan_f64_workspace_bytes", "o3dx_dbscan_f64")


# ------------------------------------------------------------ the scale case
def _fmix32(h):
    """MurmurHash3's 32-bit finalizer on a uint32 array."""
    h = h.copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def hash_points(n, seed=0x9E3779B9):
    """(n,3) float32 points in the unit cube from an integer hash of (index,
    axis): the same values everywhere, no RNG stream involved."""
    with np.errstate(over="ignore"):
        k = (np.arange(3 * n, dtype=np.uint64) + np.uint64(seed)).astype(np.uint32)
        u = _fmix32(_fmix32(k) + np.uint32(seed))
    return (u.astype(np.float64) / 4294967296.0).reshape(n, 3).astype(np.float32)


# --------------------------------------------------------- the restatement
def d2_exact(a, b):
    """sklearn's KD-tree rdist: ((dx dx) + dy dy) + dz dz in float64."""
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def pairs_dense(p, eps, chunk=512):
    """Every directed pair (i, j), i == j included, with d^2 <= eps^2: brute force."""
    p = np.asarray(p, np.float64)
    ii, jj = [], []
    for s in range(0, len(p), chunk):
        a, b = np.nonzero(d2_exact(p[s:s + chunk, None, :], p[None, :, :]) <= eps * eps)
        ii.append((a + s).astype(np.int32))
        jj.append(b.astype(np.int32))
    return np.concatenate(ii), np.concatenate(jj)


def pairs_grid(p, eps):
    """pairs_dense for large n: candidates from a cell grid (cells wider than
    eps, so a pair's cells are adjacent), every pair decided by the same d^2."""
    p = np.asarray(p, np.float64)
    n = len(p)
    c = np.floor((p - p.min(0)) / (eps * 1.001)).astype(np.int64) + 1
    dims = c.max(0) + 2
    key = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    order = np.argsort(key, kind="stable")
    skey = key[order]
    ii, jj = [], []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                nk = key + (dz * dims[1] + dy) * dims[0] + dx
                lo, hi = np.searchsorted(skey, nk, "left"), np.searchsorted(skey, nk, "right")
                cnt = hi - lo
                i = np.repeat(np.arange(n), cnt)
                pos = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(lo, cnt)
                j = order[pos]
                keep = d2_exact(p[i], p[j]) <= eps * eps
                ii.append(i[keep])
                jj.append(j[keep])
    return np.concatenate(ii), np.concatenate(jj)


def dbscan_restate(p, eps, min_samples, pairs=None):
    """(labels int32, core bool) by rules 1-5."""
    p = np.asarray(p, np.float64)
    n = len(p)
    i, j = pairs if pairs is not None else (pairs_dense(p, eps) if n <= 5000 else pairs_grid(p, eps))
    core = np.bincount(i, minlength=n) >= min_samples  # rule 2 (self counted)
    cc = core[i] & core[j]
    ei, ej = i[cc], j[cc]
    lab = np.arange(n)  # rule 3: min-index propagation with pointer jumping
    while True:
        new = lab.copy()
        np.minimum.at(new, ei, lab[ej])
        new = new[new]
        if np.array_equal(new, lab):
            break
        lab = new
    roots = core & (lab == np.arange(n))
    rank = np.cumsum(roots) - 1
    labels = np.where(core, rank[lab], -1)
    bc = ~core[i] & core[j]  # rule 4
    best = np.full(n, np.iinfo(np.int64).max)
    np.minimum.at(best, i[bc], labels[j[bc]])
    labels = np.where(~core & (best < n), best, labels)
    return labels.astype(np.int32), core


# ------------------------------------------------------------------ fixture
_cache = {}


def case(name):
    """dict(pts, eps, min_samples, labels int32, core bool[, labels_f32]) of a fixture case."""
    if name in _cache:
        return _cache[name]
    if "z" not in _cache:
        _cache["z"] = np.load(GOLDEN)
    z = _cache["z"]
    n = int(z[f"{name}_n"])
    c = dict(pts=z[f"{name}_pts"] if name in STORED else hash_points(n), eps=float(z[f"{name}_eps"]),
             min_samples=int(z[f"{name}_ms"]), labels=z[f"{name}_labels"].astype(np.int32),
             core=np.unpackbits(z[f"{name}_core"])[:n].astype(bool))
    if name == "wide":
        c["labels_f32"] = z["wide_labels_f32"].astype(np.int32)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _cache[name] = c
    return c


def n_clusters(labels):
    return int(labels.max()) + 1


# -------------------------------------------------------------------- tests
def test_surface_and_symbols():
    assert callable(getattr(o3p.PointCloud, "DBSCAN", None))
    assert callable(getattr(o3p.ops, "dbscan", None))
    header = open(N.HEADER_PATH).read()
    L = N.load()
    for s in SYMBOLS:
        assert f"{s}(" in header, s
        assert s in N.declared_symbols(), s
        assert hasattr(L, s), s
    assert L.o3dx_abi_version() == 7


@pytest.mark.parametrize("fn,wsfn", [("o3dx_dbscan", "o3dx_dbscan_workspace_bytes"),
                                     ("o3dx_dbscan_f64", "o3dx_dbscan_f64_workspace_bytes")])
def test_entry_points_validate_before_touching_the_device(fn, wsfn):
    """-EINVAL / -ENOMEM with a message for each bad argument, before any
    device call (so this runs without a GPU)."""
    L = N.load()
    f, need = getattr(L, fn), getattr(L, wsfn)
    v = ctypes.c_void_p(8)  # never dereferenced: the checks come first
    big = 1 << 40
    assert need(1000) > 0 and need(1000) >= 1000 * 17
    assert need(0) == 0 and need(1 << 31) == 0
    bad = [
        (v, 0, 0.1, 3, v, None, v, v, big),         # n <= 0
        (v, -5, 0.1, 3, v, None, v, v, big),
        (v, 1 << 31, 0.1, 3, v, None, v, v, big),   # n >= 2^31
        (v, 100, 0.0, 3, v, None, v, v, big),       # eps <= 0
        (v, 100, -1.0, 3, v, None, v, v, big),
        (v, 100, float("nan"), 3, v, None, v, v, big),
        (v, 100, float("inf"), 3, v, None, v, v, big),
        (v, 100, 0.1, 0, v, None, v, v, big),       # min_samples < 1
        (None, 100, 0.1, 3, v, None, v, v, big),    # null points
        (v, 100, 0.1, 3, None, None, v, v, big),    # null labels
        (v, 100, 0.1, 3, v, None, None, v, big),    # null n_clusters_host
    ]
    for a in bad:
        rc = f(*a, None)
        assert rc == -22 and fn.encode() in L.o3dx_last_error(), a
    for ws, nbytes in ((v, 16), (v, need(100) - 1), (None, big)):
        rc = f(v, 100, 0.1, 3, v, None, v, ws, nbytes, None)
        assert rc == -12 and b"workspace" in L.o3dx_last_error()


def test_pointcloud_dbscan_rejects_bad_input_without_a_gpu():
    pts = np.random.default_rng(0).random((50, 3))
    pc = o3p.PointCloud(pts)
    for kw in (dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")), dict(min_samples=0), dict(min_samples=-3)):
        with pytest.raises(ValueError):
            pc.DBSCAN(**kw)
    with pytest.raises(ValueError):
        o3p.PointCloud().DBSCAN()
    with pytest.raises(ValueError):
        o3p.PointCloud(np.zeros((0, 3))).DBSCAN()
    for badv in (np.nan, np.inf):
        q = pts.copy()
        q[7, 1] = badv
        with pytest.raises(ValueError):
            o3p.PointCloud(q).DBSCAN(0.1, 3)
        with pytest.raises(ValueError):
            o3p.PointCloud(torch.as_tensor(q)).DBSCAN(0.1, 3)
    with pytest.raises(ValueError):
        o3p.ops.dbscan(torch.zeros((4, 3)), 0.0, 3)
    with pytest.raises(ValueError):
        o3p.ops.dbscan(torch.zeros((4, 3)), 0.1, 0)
    with pytest.raises(ValueError):
        o3p.ops.dbscan(torch.zeros((0, 3)), 0.1, 3)
    if not torch.cuda.is_available():  # no CPU fallback
        with pytest.raises(RuntimeError):
            pc.DBSCAN(0.1, 3)
        with pytest.raises(RuntimeError):
            o3p.ops.dbscan(torch.zeros((4, 3)), 0.1, 3)


def test_fixture_shapes():
    assert os.path.getsize(GOLDEN) < 1 << 20
    want = dict(uniform=(4000, 0.06, 5), blobs=(3200, 0.04, 6), lattice=(400, 1.0, 4), dups=(900, 0.05, 4),
                chain=(3000, 0.0125, 3), wide=(2500, 0.04, 6))
    for name, (n, eps, ms) in want.items():
        c = case(name)
        assert c["pts"].shape == (n, 3) and c["eps"] == eps and c["min_samples"] == ms, name
        assert c["labels"].shape == (n,) and c["core"].shape == (n,)
        assert c["pts"].dtype == (np.float64 if name == "wide" else np.float32)
    s = case("scale")
    assert len(s["pts"]) in (100000, 50000) and s["min_samples"] == 5 and n_clusters(s["labels"]) >= 2000
    assert n_clusters(case("blobs")["labels"]) == 4 and (case("blobs")["labels"] == -1).any()
    assert n_clusters(case("chain")["labels"]) == 1 and case("chain")["core"].sum() == 2998  # the two ends
    assert n_clusters(case("uniform")["labels"]) > 50
    w = case("wide")  # narrowing the wide cloud to float32 changes the labels
    assert not np.array_equal(w["labels"], w["labels_f32"])


def test_fixture_exercises_what_it_is_for():
    u = case("uniform")  # border points with two candidate clusters
    i, j = pairs_dense(u["pts"], u["eps"])
    bc = ~u["core"][i] & u["core"][j]
    lo = np.full(len(u["pts"]), 1 << 30)
    hi = np.full(len(u["pts"]), -1)
    np.minimum.at(lo, i[bc], u["labels"][j[bc]])
    np.maximum.at(hi, i[bc], u["labels"][j[bc]])
    assert int(((hi > lo) & (hi >= 0)).sum()) >= 10
    lat = case("lattice")  # pairs at d^2 == eps^2 exactly
    i, j = pairs_dense(lat["pts"], lat["eps"])
    d2 = d2_exact(lat["pts"][i].astype(np.float64), lat["pts"][j].astype(np.float64))
    assert (d2 == lat["eps"] ** 2).sum() > 400
    d = case("dups")  # d^2 == 0 between distinct points
    i, j = pairs_dense(d["pts"], d["eps"])
    assert ((d2_exact(d["pts"][i].astype(np.float64), d["pts"][j].astype(np.float64)) == 0) & (i != j)).sum() == 1800


def test_grid_pairs_equal_dense_pairs():
    for name in ("uniform", "lattice", "dups", "wide"):
        c = case(name)
        a = np.stack(pairs_dense(c["pts"], c["eps"]), 1)
        b = np.stack(pairs_grid(c["pts"], c["eps"]), 1)
        assert np.array_equal(a[np.lexsort(a.T[::-1])], b[np.lexsort(b.T[::-1])]), name


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_fixture(name):
    """Rules 1-5 in numpy give sklearn's labels and core mask (the scale case
    through the cell-grid pair list, which the test above ties to brute force)."""
    c = case(name)
    labels, core = dbscan_restate(c["pts"], c["eps"], c["min_samples"])
    assert np.array_equal(core, c["core"])
    assert np.array_equal(labels, c["labels"])
    if name == "wide":
        l32, _ = dbscan_restate(c["pts"].astype(np.float32), c["eps"], c["min_samples"])
        assert np.array_equal(l32, c["labels_f32"])


@pytest.mark.parametrize("name", CASES)
def test_sklearn_equals_fixture(name):
    skc = pytest.importorskip("sklearn.cluster")
    c = case(name)
    m = skc.DBSCAN(eps=c["eps"], min_samples=c["min_samples"]).fit(np.asarray(c["pts"], np.float64))
    core = np.zeros(len(c["pts"]), bool)
    core[m.core_sample_indices_] = True
    assert np.array_equal(m.labels_, c["labels"]) and np.array_equal(core, c["core"])


@pytest.mark.parametrize("name", CASES)
def test_band_condition(name):
    """No pair at a distance within eps (1 +- 1e-7): sklearn's tree may accept
    a node by a bound, so such a pair would not be pinned.  (The lattice's
    coordinates and sums are exact: its pairs sit on eps exactly or far off.)"""
    c = case(name)
    p = np.asarray(c["pts"], np.float64)
    eps = c["eps"]
    i, j = (pairs_dense if len(p) <= 5000 else pairs_grid)(p, eps * (1 + 2e-7))
    d = np.sqrt(d2_exact(p[i], p[j]))
    band = (d >= eps * (1 - 1e-7)) & (d <= eps * (1 + 1e-7))
    if name == "lattice":
        assert np.array_equal(band, d == eps)
    else:
        assert not band.any()
