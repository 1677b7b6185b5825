"""CPU: the RANSAC plane cases of plane_edge_cases.py — their plain references
against the oracle, the class table and its caps, the recorded numbers of the
explicit cases, and the library's host-side selection replay (it loads without
a GPU) on the references' counts and sums."""
import math

import numpy as np
import pytest

import edge_clouds as E
import plane_edge_cases as PC
from open3dpypro import _native as N
from open3dpypro import ops
from oracle import oracle as O


@pytest.fixture(scope="module")
def oracle_results():
    """id -> O.segment_plane of every case (computed once)."""
    out = {}
    for cid, c in PC.cases().items():
        out[cid] = O.segment_plane(c.pts, c.thr, c.rn, c.H, c.samples, c.prob)
    return out


def test_case_list():
    cs = PC.cases()
    grid = PC.ids(kind="grid")
    assert len(grid) == 765 and len(PC.ids(kind="guard")) == 27
    for c in cs.values():
        assert len(c.pts) <= 12288 and len(c.pts) >= c.rn and c.samples.shape == (c.H, c.rn)
        assert c.pts.dtype == (np.float64 if c.wide else np.float32)
        assert c.H == 0 or (0 <= c.samples.min() and c.samples.max() < len(c.pts))
    assert set(PC.clouds()) == {n for n in E.names() if len(E.cloud(n)) >= 3}


def test_references_equal_the_oracle(oracle_results):
    """Counts (-1 exactly at the degenerate hypotheses), Sigma|d| to 1e-12, the
    best index and the inliers where the selection is pinned, the plane where
    the refit is conditioned; the other classes' property checks hold for the
    oracle's own results."""
    for cid, (plane, inl, counts, sums, best) in oracle_results.items():
        r = PC.reference(cid)
        assert np.array_equal(counts, r.counts), cid
        assert np.array_equal(counts < 0, ~np.any(r.planes != 0, 1)), cid
        np.testing.assert_allclose(sums, r.sums, rtol=1e-12, atol=0, err_msg=cid)
        if r.pinned:
            assert best == r.best, cid
        PC.check_result(cid, plane, inl)


def test_class_table(oracle_results):
    """The two weak classes stay small, and the Rayleigh margin is the measured one."""
    cs = PC.cases()
    unpinned = [cid for cid in cs if not PC.reference(cid).pinned]
    uncond = [cid for cid in cs if not PC.reference(cid).conditioned]
    under = [cid for cid in cs if PC.reference(cid).underflow]
    thin = [cid for cid in cs if PC.eigh_applies(cid)]
    excess = 0.0
    for cid in uncond:
        r = PC.reference(cid)
        plane, inl = oracle_results[cid][:2]
        if plane.any() and np.array_equal(inl, r.inliers):
            excess = max(excess, PC.excess_over_lambda1(r.cov, r.evals, plane))
    print(f"\nplane cases: {len(cs)}; selection unpinned: {len(unpinned)} {unpinned}; refit unconditioned: "
          f"{len(uncond)}; underflow reached: {len(under)} {under}; eigenvector reference binds: {len(thin)}; "
          f"oracle's largest Rayleigh excess over the unconditioned cases: {excess:.3e} of lambda_3")
    assert len(unpinned) <= PC.CAP_UNPINNED * len(cs)
    assert len(uncond) <= PC.CAP_UNCONDITIONED * len(cs)
    assert excess <= PC.MEASURED_RAYLEIGH_EXCESS  # the recorded figure is the largest
    assert PC.RAYLEIGH_MARGIN == max(16 * PC.MEASURED_RAYLEIGH_EXCESS, 2.0 ** -40)
    # the grid's unpinned cases: three of tiny4's four points are inliers of
    # every hypothesis and Sigma|d| is one term of rounding noise (1e-17).  On
    # wide_tiny4 those terms are multiples of the offset's ulp (2^-30 or so):
    # order-free, and the case stays pinned
    assert {c for c in unpinned if cs[c].kind == "grid"} == {f"tiny4-n3-H{H}-t0.01" for H in (64, 300)}
    assert len(thin) >= 200
    # the unconditioned families
    fam = {cs[c].cloud for c in uncond if cs[c].kind == "grid" and cs[c].H > 1}
    assert {"two_far", "wide_lattice", "wide_collapsed"} <= fam


def test_underflow_is_reached():
    for cid in PC.UNDERFLOW_GRID + ("underflow-tiny65-n16",):
        r = PC.reference(cid)
        c = PC.cases()[cid]
        assert r.underflow and r.best >= 0, cid  # some record of the replay has fitness^ransac_n < 2^-53
        assert math.pow(r.counts[r.consulted[0]] / len(c.pts), c.rn) < 2.0 ** -53
    for cid in PC.ids(cloud="wide_collapsed"):
        c = PC.cases()[cid]
        if c.rn == 6 and c.thr == 0.05 and c.H > 1:
            assert PC.reference(cid).underflow, cid


def test_recorded_numbers():
    """lattice_at_thr: 144 / 144 / 432 per hypothesis and the plane (0, 0, 1,
    -5); on wide_lattice 144 / 432 and d = -310.3125."""
    for tag, count in (("at", 144), ("below", 144), ("above", 432)):
        r = PC.reference(f"lattice_at_thr-{tag}")
        assert r.counts.tolist() == [count, count] and r.best == 0 and len(r.inliers) == count
        assert np.array_equal(r.planes, [[0, 0, 1, -5], [1, 0, 0, -3]])
        assert np.array_equal(r.plane, [0, 0, 1, -5]) and r.pinned
        assert np.array_equal(np.abs(r.plane_eigh), [0, 0, 1, 5])
    assert PC.reference("lattice_at_thr-above").sums.tolist() == [288.0, 288.0]
    for tag, count in (("at", 144), ("above", 432)):
        r = PC.reference(f"wide_lattice_at_thr-{tag}")
        assert r.counts.tolist() == [count, count] and r.best == 0 and r.pinned
        assert np.array_equal(r.planes, [[0, 0, 1, -310.3125], [1, 0, 0, -420000.1875]])
        assert np.array_equal(r.plane, [0, 0, 1, -310.3125])
    lat = np.asarray(E.cloud("lattice3d"), np.float64)
    assert np.array_equal(np.unique(lat[PC.reference("lattice_at_thr-above").inliers, 2]), [4, 5, 6])


def test_degenerate_first():
    for name in ("flatz@0", "flatx@1000.5", "lattice3d"):
        r = PC.reference(f"degenerate_first-{name}")
        assert r.counts[:3].tolist() == [-1, -1, -1] and (r.counts[3:] >= 3).all()
        if name != "lattice3d":  # the first plane holds the whole cloud: fitness 1 stops the loop
            n = len(E.cloud(name))
            assert r.best == 3 and (r.counts[3:] == n).all() and len(r.inliers) == n
            assert r.consulted.tolist() == [3] and not r.sums.any()
    r = PC.reference("degenerate_counter")
    assert r.counts.tolist() == [7 * 144, -1, -1, 11 * 144, 11 * 144]
    assert r.best == 3 and r.consulted.tolist() == [0, 3]  # a counter moved by the degenerate ones would stop at 0
    assert PC.break_iteration(7 / 12, 3, 0.25, 5) == (1, False)


def test_all_degenerate_clouds():
    """line_x and same: every hypothesis degenerate at every ransac_n — best -1, zero plane, no inliers."""
    for name in ("line_x", "same"):
        ids = PC.ids(cloud=name)
        assert len(ids) == 27
        for cid in ids:
            r = PC.reference(cid)
            assert (r.counts == -1).all() and r.best == -1 and len(r.inliers) == 0 and not r.plane.any(), cid
    for cid in PC.ids(kind="n_eq_rn"):
        if PC.cases()[cid].H == 0:
            r = PC.reference(cid)
            assert r.best == -1 and len(r.inliers) == 0 and not r.plane.any()


def test_flat_clouds_sum_to_zero():
    """Every hypothesis of a flat cloud at ransac_n 3 is the cloud's plane: Sigma|d| exactly 0."""
    for name in E.FLAT:
        for cid in PC.ids(cloud=name):
            c = PC.cases()[cid]
            r = PC.reference(cid)
            if c.rn == 3:
                assert (r.counts[r.counts >= 0] == len(c.pts)).all() and not r.sums.any(), cid


def test_order_free():
    assert PC.order_free([], 0.01) and PC.order_free([0.0, 0.0], 0.01) and PC.order_free([1.0] * 288, 1.5)
    assert PC.order_free([0.0625] * 432, 0.07) and not PC.order_free([0.1, 0.2, 0.3], 1.0)
    assert not PC.order_free([1.0, 2.0 ** -60], 1.5) and not PC.order_free([0.0, 1e-17], 0.01)


# ------------------------------------------------- the library's host code
def test_break_iteration_helper():
    """The early-stop helper of the library and of the oracle: H where the
    quotient is -inf or NaN, 0 at fitness 1, the truncated quotient otherwise."""
    N.load()
    for fn in (ops.ransac_break_iteration, O.ransac_break_iteration):
        for H in (1, 64, 300):
            assert fn(1e-4, 6, PC.PROB, H) == H          # 1e-24 < 2^-53: log(1 - 0) = +0, quotient -inf
            assert fn(0.05, 16, PC.PROB, H) == H
            assert fn(1e-4, 6, 1e-20, H) == H            # 1 - p == 1 as well: 0 / 0 = NaN
            assert fn(0.0, 3, PC.PROB, H) == H
            assert fn(1.0, 3, PC.PROB, H) == 0
            assert fn(0.5, 3, 1.0, H) == H               # log(0) = -inf: +inf, capped
        assert fn(0.5, 3, PC.PROB, 300) == int(math.log(1 - PC.PROB) / math.log(1 - 0.125)) == 137
        assert fn(0.5, 3, PC.PROB, 64) == 64
        assert fn(7 / 12, 3, 0.25, 5) == 1
        for fit, rn, p, H in ((0.3, 3, 0.99, 1000), (0.9, 5, PC.PROB, 300), (1e-3, 3, 0.5, 10 ** 9),
                              (144 / 1728, 3, PC.PROB, 2)):
            assert fn(fit, rn, p, H) == PC.break_iteration(fit, rn, p, H)[0]


def _host_replays(cid):
    c = PC.cases()[cid]
    r = PC.reference(cid)
    n = len(c.pts)
    if c.H == 0:
        return
    assert ops.ransac_select(r.counts, r.sums, r.planes, n, c.rn, c.prob) == r.best, cid
    assert np.array_equal(ops.ransac_tied(r.counts, r.planes, n, c.rn, c.prob), r.tied), cid
    none = np.zeros(c.H, bool)
    assert np.array_equal(ops.ransac_needed(r.counts, none, r.planes, n, c.rn, c.prob), r.consulted), cid
    assert len(ops.ransac_needed(r.counts, ~none, r.planes, n, c.rn, c.prob)) == 0, cid
    # upper bounds on the hypotheses the replay does not consult leave the rounds at the exact selection
    ub = r.counts.copy()
    known = np.zeros(c.H, bool)
    known[r.consulted] = True
    loose = ~known & (ub >= 0)
    ub[loose] = np.minimum(ub[loose] + (np.arange(c.H)[loose] % 3), n)
    for _ in range(c.H + 1):
        need = ops.ransac_needed(ub, known, r.planes, n, c.rn, c.prob)
        if len(need) == 0:
            break
        ub[need] = r.counts[need]
        known[need] = True
    assert len(need) == 0
    assert np.array_equal(ops.ransac_tied(ub, r.planes, n, c.rn, c.prob), r.tied), cid
    assert ops.ransac_select(ub, r.sums, r.planes, n, c.rn, c.prob) == r.best, cid


def test_host_replays_on_every_case():
    """ransac_select / ransac_tied / ransac_needed give the reference's choice,
    tie set and consulted set on every case, the underflow cases included."""
    N.load()
    for cid in PC.cases():
        _host_replays(cid)


def test_host_replays_on_an_all_n_tie():
    """Every hypothesis holds the whole cloud: fitness 1 stops the loop at the
    first non-degenerate one; below fitness 1 the whole run ties and the
    smallest Sigma|d| (the first of equal ones) wins."""
    N.load()
    H, n = 64, 1000
    planes = np.tile([0.0, 0.0, 1.0, -0.25], (H, 1))
    planes[0] = 0.0
    counts = np.full(H, n, np.int64)
    counts[0] = -1
    sums = np.zeros(H)
    assert ops.ransac_select(counts, sums, planes, n, 3) == 1 == PC.select(counts, sums, n, 3).best
    assert len(ops.ransac_tied(counts, planes, n, 3)) == 0 == len(PC.select(counts, sums, n, 3).tied)
    counts[1:] = n - 1  # fitness 0.999: the early-stop point is 3, four hypotheses are processed
    sums = np.linspace(2.0, 1.0, H)
    sel = PC.select(counts, sums, n, 3)
    assert sel.tied.tolist() == [1, 2, 3, 4] and sel.best == 4
    assert ops.ransac_tied(counts, planes, n, 3).tolist() == [1, 2, 3, 4]
    assert ops.ransac_select(counts, sums, planes, n, 3) == 4
    sel = PC.select(counts, sums, n, 3, 1.0)  # probability 1: no early stop, all of them tie
    assert sel.tied.tolist() == list(range(1, H)) and sel.best == H - 1
    assert ops.ransac_tied(counts, planes, n, 3, 1.0).tolist() == list(range(1, H))
    assert ops.ransac_select(counts, sums, planes, n, 3, 1.0) == H - 1
    assert ops.ransac_select(counts, np.ones(H), planes, n, 3, 1.0) == 1
