"""CPU checks of tests/icp_loop_cases.py: every case's reference trajectory
stays finite and small, the brute-force correspondences equal the oracle's at
every trajectory step, the parity class is what the margin rule gives, the tie
cases really tie, walk_in's rows cross the radius in both directions, and the
GPU file's parametrisation lists are what they are meant to be.
test_gpu_icp_loop_edges.py then holds the device loops to these references."""
import numpy as np
import pytest

import edge_clouds as E
import icp_loop_cases as C
from oracle import oracle as O

LOOPS = C.combos(loops=True)
IDS = [f"{n}-{e}" for n, e in LOOPS]

# with_scaling where the matched pairs have no spread (one pair, or — from
# the second update on — sources a scale of 0 collapsed onto one target):
# Eigen's umeyama divides 0 by 0 and the reference T is NaN
# (icp_loop_cases.reference_defined)
UNDEFINED = frozenset((n, "scaled") for n in
                      ("tiny_t1_s1", "tiny_t1_s2", "tiny_t1_s3", "tiny_t2_s1", "tiny_t2_s2", "tiny_t3_s1", "lattice_s1",
                       "wide_tiny_t1_s1", "wide_tiny_t1_s2", "wide_tiny_t1_s3", "wide_tiny_t2_s1", "wide_tiny_t3_s1"))


def test_cases_are_small_and_read_only():
    for c in C.cases().values():
        assert len(c.tgt) <= 12288 and len(c.src) <= 12288 and len(c.src) >= 1
        assert c.tgt.dtype == c.src.dtype == (np.float64 if c.wide else np.float32), c.name
        assert not c.tgt.flags.writeable and not c.src.flags.writeable
        assert c.tn is None or (c.tn.dtype == np.float32 and len(c.tn) == len(c.tgt))
        if c.wide:  # float32 cannot hold the cloud
            assert not np.array_equal(c.tgt.astype(np.float32).astype(np.float64), c.tgt), c.name
    assert set(E.icp_cases()) <= set(C.cases())
    for n in C.WALK_N:
        assert np.array_equal(C.cases()[f"walk_in_n{n}"].src, C.cases()["walk_in"].src[:n])


@pytest.mark.parametrize("name", ["lattice_tie", "tiny_t1_s3", "walk_in_n257", "dup_target", "wide_lattice_tie"])
def test_top2_equals_brute_table(name):
    c = C.cases()[name]
    q = E.transform_unfused(c.src[:300], c.init)
    for got, ref in zip(C.top2(c.tgt, q, chunk=128), E.brute_table(c.tgt, q, 2)):
        assert np.array_equal(got, ref)


@pytest.mark.parametrize("name,est", LOOPS, ids=IDS)
def test_reference_trajectory_is_finite_and_small(name, est):
    """A condition on the inputs: T finite and max |T_ij| <= 1e3 after every
    iteration up to the largest max_iteration of the GPU tests.  The
    combinations whose reference is NaN are exactly UNDEFINED."""
    assert C.MAX_IT == 8
    if (name, est) in UNDEFINED:
        assert not C.reference_defined(name, est)
        return
    tr = C.trajectory(name, est)
    assert len(tr) == C.MAX_IT + 1
    for m, (T, corr, fit, rm) in enumerate(tr):
        assert np.isfinite(T).all() and np.isfinite([fit, rm]).all(), (name, est, m)
        assert np.abs(T).max() <= 1e3, (name, est, m, np.abs(T).max())
    assert np.array_equal(tr[0][0], C.cases()[name].init)


@pytest.mark.parametrize("name,est", LOOPS, ids=IDS)
def test_brute_corr_equals_oracle_along_trajectory(name, est):
    """brute_corr == O.knn_search(HYBRID, 1, r) under every T of the
    trajectory; on the parity class it is the reference loop's own
    correspondence set, with its fitness and rmse."""
    if (name, est) in UNDEFINED:
        return
    c = C.cases()[name]
    for m, (T, corr, fit, rm) in enumerate(C.trajectory(name, est)):
        idx, _, cnt = O.knn_search(c.tgt, E.transform_unfused(c.src, T), O.HYBRID, 1, c.r)
        exp = np.stack([np.nonzero(cnt > 0)[0], idx[cnt > 0, 0]], 1)
        got = C.brute_corr(c, T)
        assert np.array_equal(got, exp), (name, est, m)
        if C.in_parity(name, est):
            assert np.array_equal(got, corr), (name, est, m)
            f, r, _ = C.metrics_of(c, T, got)
            assert abs(f - fit) < 1e-12 and abs(r - rm) < 1e-9, (name, est, m)


@pytest.mark.parametrize("name,est", LOOPS, ids=IDS)
def test_class_table(name, est):
    """A (case, estimation) is in the parity class exactly when every match of
    its reference trajectory is decided by more than 1e-7 max(1, |coordinates|)
    and every update solves a full-rank system.  Measured (smallest gap over
    the 9 steps):

    parity:   walk_in, every estimation (7e-7, 8e-7, 2e-7), walk_slow likewise
              (4e-7, 2e-7, 4e-7); walk_in's sub-sources of
              sub-sources of 63 to 257 rows (3e-7 and more), 1793 (point 3e-7, scaled 1.4e-7)
              and 2049 (plane 8e-7, point 3e-7); dup_target, every estimation
              (1e-2 besides its 2000 exact ties per step); lattice_tie, flat_off,
              tiny_t3_s3, lattice_s3 and the float64 wide_lattice_walk under
              point-to-point with and without scaling.
    property: walk_in_n1793 plane (6e-8) and walk_in_n2049 scaled (1e-7);
              lattice_past_r (every candidate 1e-16 inside the radius); the
              float64 clouds but one (their bar is 2e-3 at 1e4 m and 0.46 at
              4.6e6 m); everything rank-deficient: point-to-plane on the
              lattice and the flat target (all normals up), fewer than 3
              pairs, several sources on one target, lattice_at_r (no pairs)."""
    assert C.parity_rule(name, est) == C.in_parity(name, est), (name, est)


def test_parity_class_holds_what_it_must():
    ests = {e for _, e in C.PARITY}
    assert ests == set(C.ESTS)
    assert any(C.cases()[n].wide for n, _ in C.PARITY)
    assert any(n == "flat_off" for n, _ in C.PARITY)
    assert all(("walk_in", e) in C.PARITY for e in C.ESTS)
    assert C.PARITY <= set(LOOPS) and not (C.PARITY & UNDEFINED)
    for n, e in C.PARITY:
        assert C.MAX_IT in C.max_its_of(n, e, (C.MAX_IT,))


def test_tie_cases_tie():
    """dup_target (every estimation) and lattice_tie under point-to-plane have
    exact ties in every iteration; lattice_tie's T stays init bit for bit;
    lattice_at_r never has a correspondence, every candidate at exactly r."""
    for e in C.ESTS:
        assert all(t == 2000 for _, t in C.decided_margin("dup_target", e)), e
    assert all(t > 300 for _, t in C.decided_margin("lattice_tie", "plane"))
    init = C.cases()["lattice_tie"].init
    for T, corr, fit, rm in C.trajectory("lattice_tie", "plane"):
        assert np.array_equal(T, init) and len(corr) == 440 and fit == 1.0
    for e in C.ESTS:
        for T, corr, fit, rm in C.trajectory("lattice_at_r", e):
            assert len(corr) == 0 and fit == 0.0 and rm == 0.0 and np.array_equal(T, init)
        assert all(t == 440 for _, t in C.decided_margin("lattice_at_r", e))
    # the lower index of a duplicate pair lies in either half of the doubled cloud
    c = C.cases()["dup_target"]
    idx, d2 = C.table_at(c, E.transform_unfused(c.src, c.init))
    assert (d2[:, 0] == d2[:, 1]).all() and (idx[:, 0] < idx[:, 1]).all()
    assert np.array_equal(c.tgt[idx[:, 0]], c.tgt[idx[:, 1]])
    second = idx[:, 0] >= len(c.tgt) // 2  # both copies in the second half: a quarter of a random placement
    assert 0.1 < second.mean() < 0.5, second.mean()


def test_walk_in_crosses_the_radius():
    """The reference fitness starts below 0.6 and ends above 0.9 within 8
    iterations, and along the trajectory rows go unmatched -> matched and
    matched -> unmatched (under each estimation)."""
    tr = C.trajectory("walk_in", "plane")
    assert tr[0][2] < 0.6 and tr[-1][2] > 0.9, (tr[0][2], tr[-1][2])
    ns = len(C.cases()["walk_in"].src)
    for e in C.ESTS:
        gained = lost = 0
        tr = C.trajectory("walk_in", e)
        for (_, a, _, _), (_, b, _, _) in zip(tr[:-1], tr[1:]):
            ma, mb = np.zeros(ns, bool), np.zeros(ns, bool)
            ma[a[:, 0]] = True
            mb[b[:, 0]] = True
            gained += int((~ma & mb).sum())
            lost += int((ma & ~mb).sum())
        assert gained >= 1 and lost >= 1, (e, gained, lost)


def test_walk_slow_rows_leave_while_their_margin_holds():
    """walk_slow under point-to-point (with and without scaling): at steps 2
    to 6 of the reference trajectory matched rows drift out of the radius with
    the same nearest target, while their runner-up lay more than 2.2 times
    their motion beyond the match: the skip proof's margin alone would keep
    them, the d^2 < r^2 test of the kept arm lets them go.  Every row moves by
    less than half a millimetre a step from the second step on."""
    for e in ("point", "scaled"):
        steps = C.kept_rows_leaving("walk_slow", e)
        assert [k for k, _, _ in steps] == list(range(2, C.MAX_IT + 1))
        assert sum(len(r) for _, r, _ in steps) >= 10, e
        assert sum(len(r) > 0 for _, r, _ in steps) >= 4, e
        assert max(m for _, _, m in steps) < 5e-4, e


@pytest.mark.parametrize("name", sorted(C.prior_cases()))
def test_planted_priors(name):
    """What test_any_prior_gives_the_full_search plants: on the lattice the
    new step ties most rows, and the prior is the higher index of the tie for
    at least a quarter of them and the lower for at least a quarter
    (lat_low and lat_high alike: the lattice's indices are permuted); lat_far
    has priors and no match; on walk_in a good part of the priors is not the new match, rows lose and gain their match."""
    prior, (idx, d2) = C.prior_rows(name)
    cname, src, T1, T2 = C.prior_cases()[name]
    c = C.cases()[cname]
    r2 = c.r * c.r
    assert len(prior) == len(src) and prior.max() < len(c.tgt)
    if name in ("lat_low", "lat_high"):
        tied = (d2[:, 0] == d2[:, 1]) & (d2[:, 0] < r2) & (prior >= 0)
        assert tied.sum() > 300
        hi, lo = prior[tied] == idx[tied, 1], prior[tied] == idx[tied, 0]
        assert (hi | lo).all()
        assert hi.mean() >= 0.25 and lo.mean() >= 0.25, (hi.mean(), lo.mean())
    elif name == "lat_far":
        assert (prior >= 0).all() and not (d2[:, 0] < r2).any()
    else:
        has = (prior >= 0) & (d2[:, 0] < r2)
        assert has.sum() > 2000 and (prior[has] != idx[has, 0]).mean() > 0.2, (has.sum(), (prior[has] != idx[has, 0]).mean())
        assert ((prior >= 0) & ~(d2[:, 0] < r2)).any() and ((prior < 0) & (d2[:, 0] < r2)).any()


def test_shard_splits_cover():
    for name in C.SHARD_CASES:
        ns = len(C.cases()[name].src)
        for split, parts in C.shard_splits(ns).items():
            assert parts[0][0] == 0 and parts[-1][1] == ns
            assert all(a[1] == b[0] for a, b in zip(parts[:-1], parts[1:]))
            assert any(a == b for a, b in parts) == (split == "empty")
    assert sorted(b - a for a, b in C.shard_splits(3)["empty"]) == [0, 1, 2]


def test_gpu_parametrisation():
    """The GPU file's lists are non-empty and keep their lengths, and none of
    its cases carries a skip or an expected-failure mark."""
    import test_gpu_icp_loop_edges as G

    n32, n64 = len(C.names(False)), len(C.names(True))
    assert (n32, n64) == (30, 9)
    assert len(G.ALL) == len(C.combos()) == 3 * n32 + 3 * (n64 - 1) + 2 == 116
    assert len(G.ALL_LOOPS) == len(LOOPS) == 116 - 7
    assert len(G.F32_LOOPS) == 3 * n32 == 90
    assert len(G.PARITY) == len(C.PARITY) == 41
    assert len(G.PRIORS) == 4 and len(G.SHARDS) == 5 * 3
    marks = G.pytestmark if isinstance(G.pytestmark, (list, tuple)) else [G.pytestmark]
    assert [m.name for m in marks] == ["gpu"]
    for k, f in vars(G).items():
        if k.startswith("test_"):
            for m in getattr(f, "pytestmark", []):
                assert m.name == "parametrize", (k, m.name)
                for v in m.args[1]:
                    assert not hasattr(v, "marks"), (k, v)
