"""CPU checks of tests/edge_clouds.py: the plain numpy references equal the
oracle on every cloud of the catalogue, the (cloud, k) class table is what
the stability rule gives, the collapsed cloud collapses, and the dense patch
of flat_nested reaches the nested grid.  test_gpu_edges.py then holds the GPU
kernels to these references."""
import numpy as np
import pytest

import edge_clouds as E
from oracle import oracle as O
from oracle import np_restate as NPR


@pytest.mark.parametrize("name", E.names())
def test_brute_knn_equals_oracle(name):
    """brute_knn == O.knn_search, indices, d^2 and counts, for every k of the
    sweep: KNN, and HYBRID at a radius that cuts the neighbourhoods; on the
    cloud's own points and on queries outside its bounds."""
    x = E.cloud(name)
    for q in (x, E.outside_queries(x)):
        tab = E.self_table(name) if q is x else E.brute_table(x, q, 64)
        for k in E.ks_for(name):
            got = E.brute_knn(x, q, O.KNN, k, table=tab)
            ref = O.knn_search(x, q, O.KNN, k)
            for g, r in zip(got, ref):
                assert np.array_equal(g, r), (name, k)
            r_cut = E.cut_radius(got[1][:, min(k, len(x)) - 1])
            got = E.brute_knn(x, q, O.HYBRID, k, r_cut, table=tab)
            ref = O.knn_search(x, q, O.HYBRID, k, r_cut)
            for g, r in zip(got, ref):
                assert np.array_equal(g, r), (name, k, r_cut)
            if len(x) > 1 and k > 1 and q is x and name != "same":
                assert (got[2] < min(k, len(x))).any(), (name, k, "the radius does not cut")


@pytest.mark.parametrize("name", sorted(E.SIGNED))
def test_brute_normals_equal_oracle_on_signed_class(name):
    x = E.cloud(name)
    tab = E.self_table(name)
    for k in E.SIGNED[name]:
        idx, _, cnt = E.brute_knn(x, x, O.KNN, k, table=tab)
        assert np.array_equal(E.brute_normals(x, idx, cnt), O.estimate_normals(x, O.KNN, k)), (name, k)


@pytest.mark.parametrize("name", E.names())
def test_class_table(name):
    """A (cloud, k) pair is in the signed class exactly when every row is
    stable under stable_rows (each raw moment moved by up to 4 ulp, 8 times,
    no normal moving more than 1e-6).  Measured with the real generator
    (largest move of any row in brackets):

    signed:   tiny n >= 3, every k >= 3 (4e-9); flat{x,y,z}@0, every k >= 3
              (9e-16); flat{x,y,z}@1000.5, k >= 8 (1e-7); line_x, k >= 8 (0:
              its y and z moments are exact zeros, which no summation order
              moves); lattice2d, k in {5, 32, 64} (9e-16); flat_nested,
              k >= 8 (1e-7).
    property: flat*@1000.5 at k = 3, 4, 5 (19 %, 1-2 % and 0.1-0.2 % of the
              rows unstable); line_x at k = 3, 4, 5; lattice3d at every k;
              lattice2d at the other k; two_far (half its rows); same; every
              wide_* cloud at every k (raw moments of coordinates near 4.6e6:
              all rows unstable) — wide_flatz and wide_tiny, expected signed
              from numpy stand-ins, land here; so do flat*@1000.5 at k = 8
              (expected from k = 9) and line_x / lattice2d at the k above
              (expected property-only) on the signed side."""
    x = E.cloud(name)
    tab = E.self_table(name)
    for k in E.ks_for(name):
        idx, _, cnt = E.brute_knn(x, x, O.KNN, k, table=tab)
        stable = min(k, len(x)) >= 3 and bool(E.stable_rows(x, idx, k, cnt)[0].all())
        assert stable == E.is_signed(name, k), (name, k)


def test_wide_collapsed_collapses():
    """The four points of a site share one float32 proxy (p - min bound), are
    distinct in float64, and are each other's four nearest neighbours in the
    exact float64 (d^2, index) order."""
    p = E.cloud("wide_collapsed")
    assert len(p) == 6001
    prox = (p - p.min(0)).astype(np.float32)[:-1].reshape(1500, 4, 3)
    assert (prox == prox[:, :1]).all()
    assert len(np.unique(p, axis=0)) == len(p)
    idx, d2, _ = E.brute_knn(p, p[:-1], O.KNN, 4)
    assert np.array_equal(np.sort(idx, 1), (np.arange(6000) // 4 * 4)[:, None] + np.arange(4))
    assert (d2[:, 1] > 0).all() and (np.diff(d2, axis=1) >= 0).all() and (d2[:, 3] < 1e-10).all()


@pytest.mark.parametrize("name", E.names())
def test_oracle_has_the_properties(name):
    x = E.cloud(name)
    tab = E.self_table(name)
    for k in E.ks_for(name):
        cnt = np.full(len(x), min(k, len(x)))
        E.property_checks(name, O.estimate_normals(x, O.KNN, k), cnt)
    k = 16
    r = E.below_nearest_radius(tab[1][:, 1:])
    _, _, cnt = E.brute_knn(x, x, O.HYBRID, k, r, table=tab)
    E.property_checks(name, O.estimate_normals(x, O.HYBRID, k, r), cnt)


def test_flat_nested_enters_the_nested_grid():
    """normals_on_grid (csrc/grid.hip) tries the nested grid from n >= 2 *
    kNestedMinQueries = 8192 points, and nested_tiles builds it when the
    cells of >= t = ceil(4 occ) points hold >= max(4096, n / 32) points and
    the cells within two of them at most n / 2 + 4096.  With the grid rule
    restated (edge_clouds.search_grid: one cell thick, nz = 1) every point of
    the 0.02 x 0.02 patch lies in such a cell at every k of the sweep, so the
    patch needed no shrinking."""
    x = E.cloud("flat_nested")
    assert len(x) == 12288 >= 2 * 4096
    for k in E.K:
        assert E.search_grid(x, E.knn_occupancy(k))[1][2] == 1
        dense, need, nsub, cap, t, per_point = E.nested_plan(x, k)
        assert dense >= need and nsub <= cap, (k, dense, need, nsub, cap)
        assert per_point[8192:].min() >= t, (k, per_point[8192:].min(), t)


@pytest.mark.parametrize("name", sorted(E.voxel_cases()))
def test_brute_voxel_equals_oracle(name):
    x, vs = E.voxel_cases()[name]
    ref = O.voxel_down_sample(x, vs)
    assert np.array_equal(E.brute_voxel(x, vs), ref)
    assert np.array_equal(NPR.voxel_down_sample(x, vs), ref)


@pytest.mark.parametrize("name", sorted(E.icp_cases()))
def test_brute_corr_equals_oracle(name):
    tgt, _, src, T, r = E.icp_cases()[name]
    q = E.transform_unfused(src, T)
    idx, _, cnt = O.knn_search(tgt, q, O.HYBRID, 1, r)
    exp = np.stack([np.nonzero(cnt > 0)[0], idx[cnt > 0, 0]], 1)
    got = E.brute_corr(src, tgt, T, r)
    assert np.array_equal(got, exp)
    if name == "lattice_tie":  # the ties are there, and the lower index won
        d2 = E.brute_table(tgt, q, 2)[1]
        tie = d2[:, 0] == d2[:, 1]
        assert tie[:400].sum() > 300 and not tie[400:].any() and len(got) == len(src)
    if name == "lattice_at_r":
        assert len(got) == 0
    if name == "lattice_past_r":
        assert len(got) == len(src)
    if name == "flat_off":
        assert 0 < len(got) < len(src)


@pytest.mark.parametrize("name", E.MODE_CLOUDS)
def test_mode_cases_are_stable(name):
    """The HYBRID / RADIUS cases of the signed class: at least 3 reference
    neighbours in every row, every row stable, brute_normals == the oracle."""
    x = E.cloud(name)
    for mode, k, r in E.mode_cases(name):
        idx, cnt = E.mode_rows(name, mode, k, r)
        assert cnt.min() >= 3, (name, mode, k, r)
        assert E.stable_rows(x, idx, idx.shape[1], cnt)[0].all(), (name, mode, k, r)
        assert np.array_equal(E.brute_normals(x, idx, cnt), O.estimate_normals(x, mode, k, r)), (name, mode, k)


def test_lattice_radius_one_is_strict():
    """lattice3d at r = 1.0: the distance-1 neighbours are out (d^2 < r^2 is
    strict), every row holds its own point only and gets (0,0,1); at the next
    float64 they are in (4 to 7 points per row)."""
    x = E.cloud("lattice3d")
    for mode in (O.HYBRID, O.RADIUS):
        _, cnt = E.mode_rows("lattice3d", mode, 16, 1.0)
        assert (cnt == 1).all()
        assert np.array_equal(O.estimate_normals(x, mode, 16, 1.0), np.tile([0.0, 0.0, 1.0], (len(x), 1)))
        idx, cnt = E.mode_rows("lattice3d", mode, 16, float(np.nextafter(1.0, 2.0)))
        assert cnt.min() == 4 and cnt.max() == 7
        assert np.array_equal(E.brute_normals(x, idx, cnt), O.estimate_normals(x, mode, 16, float(np.nextafter(1.0, 2.0))))
        assert E.stable_rows(x, idx, idx.shape[1], cnt)[0].sum() > 500  # 552 of 1728 rows
