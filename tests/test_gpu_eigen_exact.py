"""GPU: the normals kernels' finish (covariance tail + FastEigen3x3, eigen3.hpp)
in its product formulation against the *_ref text, on the device, bit for bit
(o3dx_normal_finish_check, ref = 0 against ref = 1, int64 views); and the
smoke-shaped cloud through the one-call pipeline against the oracle."""
import numpy as np
import pytest
import torch

from open3dpypro import _native as N
from open3dpypro import ops, synthetic as S
from oracle import oracle as O
from parity import assert_normals

pytestmark = pytest.mark.gpu

KS = (3, 4, 30, 31, 64)


def _sym6(B):
    """(n,3,3) -> {xx,xy,xz,yy,yz,zz} of B B^T"""
    C = B @ B.transpose(0, 2, 1)
    return np.stack([C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]], 1)


def _outer6(v, w=1.0):
    v = np.asarray(v, np.float64)
    w = np.broadcast_to(np.asarray(w, np.float64), v.shape[:1])[:, None]
    return w * np.stack([v[:, 0] * v[:, 0], v[:, 0] * v[:, 1], v[:, 0] * v[:, 2], v[:, 1] * v[:, 1],
                         v[:, 1] * v[:, 2], v[:, 2] * v[:, 2]], 1)


def _nudge(rng, c):
    """Non-zero entries moved by one ulp either way.  (A zero stays: its
    neighbour is the smallest subnormal, and a matrix whose largest entry is
    that overflows in the normalisation to NaNs of both signs, after which
    the bits are the compiler's operand order and not the formulation's.)"""
    return np.where(c != 0, np.nextafter(c, rng.choice([-np.inf, np.inf], c.shape)), c)


def covariance_cases(rng, per):
    """The solver's case families as covariances {xx,xy,xz,yy,yz,zz}."""
    eye = np.array([1.0, 0, 0, 1.0, 0, 1.0])
    out = []
    # random SPD, thin slabs included
    B = rng.uniform(-1, 1, (per, 3, 3))
    B[:, :, 2] *= np.ldexp(1.0, -rng.integers(0, 30, per))[:, None]
    out.append(_sym6(B))
    # rank 1 and rank 2, random and small-integer directions
    v = rng.uniform(-1, 1, (per, 3))
    v[::2] = rng.integers(-3, 4, (per, 3))[::2]
    w = rng.uniform(-1, 1, (per, 3)) * (rng.integers(0, 2, per)[:, None])
    out.append(_outer6(v) + _outer6(w))
    # all zero (either sign) and diagonal (norm == 0), equal entries included
    d = np.zeros((per, 6))
    e = rng.uniform(0, 1, (per, 3))
    e[::2, 1] = e[::2, 0]
    e[::4, 2] = e[::4, 0]
    d[:, [0, 3, 5]] = e
    d[:64] = np.where((np.arange(64)[:, None] >> np.arange(6)) & 1, -0.0, 0.0)
    out.append(d)
    # two and three equal eigenvalues (half_det = +-1): a I + b v v^T, exact small integers, some nudged
    a = rng.integers(0, 16, per) * 0.25
    b = rng.choice([0.0, -0.125, 0.5, 1.0, 1.5, 2.0], per)
    c = a[:, None] * eye + _outer6(rng.integers(-3, 4, (per, 3)), b)
    nud = rng.integers(0, 2, per).astype(bool)
    c[nud] = _nudge(rng, c[nud])
    out.append(c)
    # half_det = 0: q I + t (u u^T - w w^T), orthogonal integer u, w
    pairs = np.array([[[1, 1, 0], [1, -1, 0]], [[1, 0, 1], [1, 0, -1]], [[0, 1, 1], [0, 1, -1]],
                      [[1, 1, 1], [1, -1, 0]]], np.float64)
    p = pairs[rng.integers(0, 4, per)]
    t = rng.integers(1, 9, per) * 0.25
    c = (rng.integers(0, 9, per) * 0.5)[:, None] * eye
    c = c + _outer6(p[:, 0], t / (p[:, 0] ** 2).sum(1)) + _outer6(p[:, 1], -t / (p[:, 1] ** 2).sum(1))
    c[::2] = _nudge(rng, c[::2])
    out.append(c)
    # imax ties and |e0[0]| == |e0[1]|: symmetric under a permutation of two axes
    a = np.where(rng.integers(0, 2, per), rng.integers(0, 9, per).astype(np.float64), rng.uniform(1, 2, per))
    b = np.where(rng.integers(0, 2, per), rng.integers(-3, 4, per).astype(np.float64), rng.uniform(-1, 1, per))
    cc = np.where(rng.integers(0, 4, per) == 0, b, rng.uniform(-1, 1, per))
    e = np.where(rng.integers(0, 4, per) == 0, a, rng.uniform(1, 2, per))
    forms = [np.stack(x, 1) for x in ((a, b, cc, a, cc, e), (a, cc, b, e, cc, a), (e, cc, cc, a, b, a))]
    sel = rng.integers(0, 3, per)
    out.append(np.choose(sel[:, None], forms))
    c = np.concatenate(out)
    # entries scaled by 2^+-40 (a quarter each)
    s = rng.integers(0, 4, len(c))
    return c * np.where(s == 0, np.ldexp(1.0, 40), np.where(s == 1, np.ldexp(1.0, -40), 1.0))[:, None]


def moment_cases(rng, k, per):
    """Moment sets {x,y,z,xx,xy,xz,yy,yz,zz} of k float32 points, five families."""
    sets = []
    base = rng.uniform(0, 1, (5, per, k, 3)).astype(np.float32)
    base[1] += np.float32(5e5)
    base[2] = base[2][:, :1]
    o, dvec = base[3][:, :1], rng.uniform(-1, 1, (per, 1, 3)).astype(np.float32)
    base[3] = o + rng.uniform(-1, 1, (per, k, 1)).astype(np.float32) * dvec
    ax = rng.integers(0, 3, per)
    lvl = np.where(rng.integers(0, 2, per), 0.0, rng.uniform(-1, 1, per)).astype(np.float32)
    base[4][np.arange(per), :, ax] = lvl[:, None]
    for p in base:
        x = p.astype(np.float64)
        sets.append(np.concatenate([x.sum(1), (x[:, :, [0, 0, 0, 1, 1, 2]] * x[:, :, [0, 1, 2, 1, 2, 2]]).sum(1)], 1))
    return np.concatenate(sets)


def finish(mom, k, ref, dev):
    m = torch.from_numpy(np.ascontiguousarray(mom, np.float64)).to(dev)
    cov = torch.empty((len(mom), 6), dtype=torch.float64, device=dev)
    vec = torch.empty((len(mom), 3), dtype=torch.float64, device=dev)
    N.check(N.load().o3dx_normal_finish_check(N.ptr(m), len(mom), k, ref, N.ptr(cov), N.ptr(vec), N.stream_ptr(dev)),
            "normal_finish_check")
    return cov, vec


@pytest.fixture(scope="module")
def cases():
    rng = np.random.default_rng(11)
    per = 100_000 // 6 + 1
    c = covariance_cases(rng, per)
    # zero-mean moment sets of 4 points whose covariance is c exactly (4 c / 4)
    mom = {4: np.concatenate([np.zeros((len(c), 3)), 4.0 * c], 1)}
    for k in KS:
        mk = moment_cases(rng, k, 4000)
        mom[k] = np.concatenate([mom[k], mk]) if k in mom else mk
    return mom


def test_product_finish_equals_ref_bitwise(cases, dev):
    total, bad = 0, {}
    for k, mom in cases.items():
        cov0, vec0 = finish(mom, k, 0, dev)
        cov1, vec1 = finish(mom, k, 1, dev)
        # the solver-only entry runs the product formulation as well
        vec2 = torch.empty_like(vec0)
        N.check(N.load().o3dx_fast_eigen3x3(N.ptr(cov1), len(mom), N.ptr(vec2), N.stream_ptr(dev)), "fast_eigen")
        torch.cuda.synchronize()
        dc = (cov0.view(torch.int64) != cov1.view(torch.int64)).any(1)
        dv = (vec0.view(torch.int64) != vec1.view(torch.int64)).any(1)
        d2 = (vec2.view(torch.int64) != vec1.view(torch.int64)).any(1)
        nan_only = int((dv & torch.isnan(vec0).all(1) & torch.isnan(vec1).all(1)).sum())
        print(f"k={k}: sets={len(mom)} differing cov6={int(dc.sum())} vec3={int(dv.sum())} (all-NaN rows among them "
              f"{nan_only}) fast_eigen3x3={int(d2.sum())}")
        if bool((dc | dv | d2).any()):
            bad[k] = (int(dc.sum()), int(dv.sum()), int(d2.sum()), torch.nonzero(dc | dv | d2)[:5].flatten().tolist())
        total += len(mom)
    assert total >= 200_000
    assert not bad, bad


def test_check_entry_validates(dev):
    L = N.load()
    one = torch.zeros(9, dtype=torch.float64, device=dev)
    assert L.o3dx_normal_finish_check(N.ptr(one), 1, 0, 0, N.ptr(one), N.ptr(one), None) != 0  # k < 1
    assert L.o3dx_normal_finish_check(None, 1, 3, 0, N.ptr(one), N.ptr(one), None) != 0
    assert L.o3dx_normal_finish_check(None, 0, 3, 0, None, None, None) == 0  # nothing to do


def test_smoke_cloud_normals_within_tolerance_of_oracle(dev):
    pts = S.uniform_cube(20000, seed=3)
    vs = S.voxel_size_for(20000)
    out = ops.voxel_down_sample_normals(pts.to(dev), vs, knn=30)
    ref = O.voxel_down_sample(pts.numpy(), vs)
    assert np.array_equal(out["rep_idx"].cpu().numpy(), ref)
    reps = pts.numpy()[ref]
    exp = O.estimate_normals(reps, O.KNN, 30)
    info = assert_normals(out["normals"].cpu().numpy(), exp, reps, k=30, what="eigen_exact_smoke_cloud")
    print(info)
