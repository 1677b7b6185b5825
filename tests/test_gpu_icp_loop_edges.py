"""The ICP loops (o3dx_icp_register_est[_f64], o3dx_registration_icp_est[_f64],
o3dx_icp_shard_*) on ties, degenerate systems and tiny clouds: the state they
carry between steps — the previous matches as search priors, the skip proof's
margins and match cache, the solve and the convergence test on the device — on
exact distance ties, zero correspondences, rank-deficient systems, sources
below a wave or a block, rows that cross the radius between steps, float64
targets, and the sharded loop's digit arithmetic in one process.

The cases and the plain reference loops are tests/icp_loop_cases.py;
test_icp_loop_cases.py shows on the CPU that the references hold together and
which (case, estimation) pairs may be compared at a tolerance.  Everything
else here is bit equality: with brute force, with the host loop, between the
skip proof and the full search."""
import numpy as np
import pytest
import torch

import icp_loop_cases as C
from oracle import oracle as O
from open3dpypro import _native as N
from open3dpypro import ops

pytestmark = pytest.mark.gpu

ALL = C.combos()
ALL_LOOPS = C.combos(loops=True)
F32_LOOPS = C.combos(wide=False, loops=True)
PARITY = sorted(C.PARITY)
PRIORS = sorted(C.prior_cases())
SHARDS = [(n, s) for n in C.SHARD_CASES for s in ("two", "three", "empty")]
M_HOST = 5  # the host-loop and sharded comparisons; the skip and parity runs take C.MAX_IT


def _ids(pairs):
    return [f"{a}-{b}" for a, b in pairs]


def _t(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)  # a copy: the catalogue's arrays are read-only


def _pairs(corr):
    c = corr.cpu().numpy().astype(np.int64).reshape(-1, 2)
    return c[np.argsort(c[:, 0], kind="stable")]


_TARGETS = {}


def _target(case, dev, normals=None):
    """The case's ICPTarget (built once per target cloud, normals and radius)."""
    tn = case.tn if normals is None else normals
    key = (id(case.tgt), None if tn is None else id(tn), case.r)
    if key not in _TARGETS:
        _TARGETS[key] = (ops.ICPTarget(_t(case.tgt, dev), None if tn is None else _t(tn, dev), case.r), case.tgt, tn)
    return _TARGETS[key][0]


def _kw(est):
    e, ws = C.ESTS[est]
    return dict(estimation=e, with_scaling=ws)


def _absmax(src):
    return np.abs(np.asarray(src, np.float64)).max(0)


def _same(a, b, what):
    assert np.array_equal(a["transformation"], b["transformation"]), what
    assert a["fitness"] == b["fitness"] and a["inlier_rmse"] == b["inlier_rmse"], what
    assert np.array_equal(_pairs(a["correspondence_set"]), _pairs(b["correspondence_set"])), what


# ------------------------------------------------------------ final state
@pytest.mark.parametrize("name,est", ALL, ids=_ids(ALL))
def test_final_state_is_the_brute_force_state(dev, name, est):
    """ICPTarget.register(want_corr=True) for max_iteration 0, 1 and 5, with
    and without an early stop: the returned correspondence set is
    brute_corr(src, tgt, T_out, r) exactly, fitness = len(corr) / ns, rmse^2
    len(corr) the brute-force sum of d^2 (the bar of
    test_gpu_edges.test_icp_correspondences); zero correspondences give
    fitness 0 and rmse 0; max_iteration 0 returns init bit for bit, and so
    does lattice_tie under point-to-plane (residual exactly 0) at every
    max_iteration."""
    case = C.cases()[name]
    target = _target(case, dev)
    assert target.f64 == case.wide
    s = _t(case.src, dev)
    ns = len(case.src)
    for mi in C.max_its_of(name, est):
        for rel in (0.0, 1e-6):
            res = target.register(s, init=case.init, max_iteration=mi, relative_fitness=rel, relative_rmse=rel,
                                  want_corr=True, **_kw(est))
            tag = (name, est, mi, rel)
            T = res["transformation"]
            assert np.isfinite(T).all() and np.isfinite([res["fitness"], res["inlier_rmse"]]).all(), tag
            exp = C.brute_corr(case, T)
            assert np.array_equal(_pairs(res["correspondence_set"]), exp), tag
            assert res["fitness"] == len(exp) / ns, tag
            _, _, sd2 = C.metrics_of(case, T, exp)
            np.testing.assert_allclose(res["inlier_rmse"] ** 2 * len(exp), sd2, rtol=1e-9, atol=1e-9)
            if len(exp) == 0:
                assert res["fitness"] == 0.0 and res["inlier_rmse"] == 0.0, tag
            if mi == 0 or (name == "lattice_tie" and est == "plane"):
                assert np.array_equal(T, case.init), tag
            if name == "lattice_at_r":
                assert len(exp) == 0 and np.array_equal(T, case.init), tag


# -------------------------------------------------- device loop, host loop
def _host_loop(target, s, case, est, rel, am, max_iteration):
    """The loop over accumulate + icp_update (the multi-GPU loop's arithmetic),
    icp_metrics' rule for zero correspondences."""
    e, ws = C.ESTS[est]
    ns = len(case.src)

    def evaluate(T):
        sums, corr = target.accumulate(s, T, absmax=am, want_corr=True, estimation=e)
        if sums[28] <= 0:
            return sums, corr, 0.0, 0.0
        return sums, corr, sums[28] / ns, np.sqrt(sums[29] / sums[28])

    T = np.array(case.init, np.float64)
    sums, corr, fit, rm = evaluate(T)
    for _ in range(max_iteration):
        T = ops.icp_update(sums, T, estimation=e, with_scaling=ws)
        pf, pr = fit, rm
        sums, corr, fit, rm = evaluate(T)
        if abs(pf - fit) < rel and abs(pr - rm) < rel:
            break
    return {"transformation": T, "fitness": fit, "inlier_rmse": rm, "correspondence_set": corr}


@pytest.mark.parametrize("name,est", F32_LOOPS, ids=_ids(F32_LOOPS))
def test_device_loop_equals_host_loop(dev, monkeypatch, name, est):
    """As test_gpu_kernels.test_icp_device_loop_equals_host_loop on every
    float32 case: T, fitness, rmse and the correspondence set of the device
    loop equal the host loop's to the bit, for the caller-order and the
    spatially sorted source, with and without an early stop, with the skip
    proof and without; registration_icp in one call gives the same bits."""
    case = C.cases()[name]
    target = _target(case, dev)
    sd = _t(case.src, dev)
    am = _absmax(case.src)
    tn = None if case.tn is None else _t(case.tn, dev)
    for rel in (0.0, 1e-6):
        ref = None
        for form, s in (("caller", sd), ("sorted", ops.spatial_sort(sd))):
            host = _host_loop(target, s, case, est, rel, am, M_HOST)
            if ref is not None:  # the fx sums do not depend on the source's order
                _same(host, ref, (name, est, rel, "host loops"))
            ref = host
            for skip in ("1", "0"):
                monkeypatch.setenv("O3DX_ICP_SKIP", skip)
                res = target.register(s, init=case.init, max_iteration=M_HOST, relative_fitness=rel,
                                      relative_rmse=rel, absmax=am, want_corr=True, **_kw(est))
                _same(res, host, (name, est, rel, form, skip))
        for skip in ("1", "0"):
            monkeypatch.setenv("O3DX_ICP_SKIP", skip)
            one = ops.registration_icp(sd, _t(case.tgt, dev), tn, case.r, init=case.init, max_iteration=M_HOST,
                                       relative_fitness=rel, relative_rmse=rel, **_kw(est))
            _same(one, ref, (name, est, rel, "one call", skip))


# ------------------------------------------------------------- skip proof
@pytest.mark.parametrize("name,est", ALL_LOOPS, ids=_ids(ALL_LOOPS))
def test_skip_proof_equals_full_search(dev, monkeypatch, name, est):
    """T, fitness, rmse and the correspondences of the loop with the skip
    proof equal those of the loop that searches every step (O3DX_ICP_SKIP=0)
    to the bit, after 8 iterations with no early stop and with one: the
    caller-order source, the sorted one (spatial_sort / spatial_sort_f64) and
    the one-call form.  (On an exact tie the margin is 0: the proof never
    keeps such a match.)  No query counts, except on walk_slow, whose rows
    leave the radius while their margin holds
    (test_icp_loop_cases.test_walk_slow_rows_leave_while_their_margin_holds):
    there the proof must have kept matches, or the case checks nothing."""
    case = C.cases()[name]
    target = _target(case, dev)
    sd = _t(case.src, dev)
    td = _t(case.tgt, dev)
    tn = None if case.tn is None else _t(case.tn, dev)
    sort = ops.spatial_sort_f64 if case.wide else ops.spatial_sort
    for rel in (0.0, 1e-6):
        kw = dict(init=case.init, max_iteration=C.MAX_IT, relative_fitness=rel, relative_rmse=rel, **_kw(est))
        runs, searched = {}, {}
        for skip in ("1", "0"):
            monkeypatch.setenv("O3DX_ICP_SKIP", skip)
            N.search_stats(True)
            first = target.register(sd, want_corr=True, **kw)
            searched[skip] = N.search_stats()["queries"]
            N.search_stats(False)
            runs[skip] = [first, target.register(sort(sd), want_corr=True, **kw),
                          ops.registration_icp(sd, td, tn, case.r, **kw)]
        if name == "walk_slow" and rel == 0.0:
            assert searched["0"] >= (C.MAX_IT + 1) * len(case.src) and searched["1"] < 0.8 * searched["0"], searched
        for form, a, b in zip(("caller", "sorted", "one call"), runs["1"], runs["0"]):
            _same(a, b, (name, est, rel, form))
        for other in runs["0"][1:]:  # the three forms agree as well (order-free sums)
            _same(other, runs["0"][0], (name, est, rel, "forms"))


# ----------------------------------------------------------------- parity
_WORST = {}


@pytest.mark.parametrize("name,est", PARITY, ids=_ids(PARITY))
def test_reference_parity(dev, name, est):
    """The parity class against the reference loop (oracle.registration_icp;
    np_registration_icp_p2p over brute force) after 8 iterations, no early
    stop: T within 1e-5, fitness and rmse within 1e-6 (the project's ICP bars;
    test_gpu_icp_p2p.test_p2p_f64's for float64 point-to-point), the same
    number of correspondences — and, every match being decided, the same set."""
    case = C.cases()[name]
    target = _target(case, dev)
    res = target.register(_t(case.src, dev), init=case.init, max_iteration=C.MAX_IT, relative_fitness=0.0,
                          relative_rmse=0.0, want_corr=True, **_kw(est))
    T, corr, fit, rm = C.trajectory(name, est)[C.MAX_IT]
    dT = float(np.abs(res["transformation"] - T).max())
    df, dr = abs(res["fitness"] - fit), abs(res["inlier_rmse"] - rm)
    _WORST[(name, est)] = (dT, df, dr)
    w = [max(v[k] for v in _WORST.values()) for k in range(3)]
    print(f"parity {name} {est}: max |T - ref| {dT:.2e}, |fitness - ref| {df:.2e}, |rmse - ref| {dr:.2e}, "
          f"{len(corr)} correspondences; largest so far {w[0]:.2e} {w[1]:.2e} {w[2]:.2e}")
    np.testing.assert_allclose(res["transformation"], T, rtol=0, atol=1e-5)
    assert df < 1e-6 and dr < 1e-6
    assert len(res["correspondence_set"]) == len(corr)
    assert np.array_equal(_pairs(res["correspondence_set"]), corr)


# ---------------------------------------------------------- planted priors
def _digit_values(lo_hi):
    return [int(hi) * 2 ** 32 + int(lo) for lo, hi in lo_hi]


@pytest.mark.parametrize("skip", ["1", "0"])
@pytest.mark.parametrize("name", PRIORS)
def test_any_prior_gives_the_full_search(dev, monkeypatch, name, skip):
    """nn_search_dev's "any real point gives a valid bound": a step under T1
    leaves its matches in mpos; a second o3dx_icp_shard_begin on the same
    workspace sets T2 and leaves mpos alone; the next step starts every search
    from those planted priors — one member of the new exact tie (the lower
    index for some rows, the higher for others), the other member, a point far
    outside the radius, the matches of an unrelated motion.  Its digits equal
    the exact fx rows of a search without priors (accumulate) and the
    oracle's, and sums[28] is the brute-force count.  The lattice carries a
    different normal on every point here, so the moments tell the members of
    a tie apart.  Both steps use one target object: every planted prior is a
    row of it."""
    monkeypatch.setenv("O3DX_ICP_SKIP", skip)
    cname, src, T1, T2 = C.prior_cases()[name]
    case = C.cases()[cname]
    tn = C.prior_normals(cname)
    target = _target(case, dev, tn)
    am = _absmax(src)
    sd = _t(src, dev)
    exp = C.brute_corr(case, T2, src)
    for form, s in (("caller", sd), ("sorted", ops.spatial_sort(sd))):
        loop = ops.ICPShardLoop(s, am, case.r, init=T1)
        digits = torch.zeros(64, dtype=torch.int64, device=dev)
        loop.step(target, digits, use_prior=False)
        first = digits.cpu().numpy().copy()
        T2c, amc = np.ascontiguousarray(T2, np.float64), np.ascontiguousarray(am, np.float64)
        N.check(loop.L.o3dx_icp_shard_begin(ops._np_ptr(T2c), ops._np_ptr(amc), loop.mc, loop.ns, N.ptr(loop.ws),
                                            loop.ws.numel(), loop.st), "icp_shard_begin")
        loop.step(target, digits, use_prior=True)
        dig = digits.cpu().numpy()
        for T, d in ((T1, first), (T2, dig)):
            sums, corr, fx = target.accumulate(s, T, absmax=am, want_corr=True, return_fx=True)
            got = _digit_values(zip(d[0::2], d[1::2]))
            assert got == _digit_values(fx[:, :2]), (name, form, "accumulate")
            rfx = O.icp_accumulate_fx(src, case.tgt, tn, case.r, T, am)
            assert np.array_equal(fx[:, 2], rfx[:, 2]) and got == _digit_values(rfx[:, :2]), (name, form, "oracle")
        assert np.array_equal(_pairs(corr), exp), (name, form)
        row = np.array([[dig[56], dig[57], fx[28, 2], 0]], np.int64)
        assert ops.fx_to_double(row)[0] == len(exp) == sums[28], (name, form)
    if name == "lat_far":
        assert len(exp) == 0


# ------------------------------------------------------------ sharded loop
@pytest.mark.parametrize("skip", ["1", "0"])
@pytest.mark.parametrize("name,split", SHARDS, ids=_ids(SHARDS))
def test_sharded_loop_in_one_process(dev, monkeypatch, name, split, skip):
    """One ICPShardLoop per shard of the source (2 shards, 3 shards, one of
    them empty) on the shared target, with the global absmax and n_total; per
    iteration every shard's step into its own digits, a torch sum, every
    shard's finish on the sum.  Every shard ends in the same state, which is
    ICPTarget.register's on the whole source in T, fitness and rmse and the
    one-shard loop's in the iterations applied, bit for bit."""
    monkeypatch.setenv("O3DX_ICP_SKIP", skip)
    case = C.cases()[name]
    target = _target(case, dev)
    ns = len(case.src)
    am = _absmax(case.src)
    parts = C.shard_splits(ns)[split]

    def run(ranges, rel, sort):
        shards = [_t(case.src[a:b], dev) for a, b in ranges]
        shards = [ops.spatial_sort(x) if sort and x.shape[0] else x for x in shards]
        loops = [ops.ICPShardLoop(x, am, case.r, init=case.init) for x in shards]
        digs = [torch.zeros(64, dtype=torch.int64, device=dev) for _ in loops]
        for it in range(M_HOST + 1):
            for lp, d in zip(loops, digs):
                lp.step(target, d, use_prior=it > 0)
            total = torch.stack(digs).sum(0)
            for lp in loops:
                lp.finish(total, ns, it, M_HOST, rel, rel, target)
        return [lp.state() for lp in loops]

    for rel in (0.0, 1e-6):
        whole = target.register(_t(case.src, dev), init=case.init, max_iteration=M_HOST, relative_fitness=rel,
                                relative_rmse=rel, absmax=am)
        (T1, f1, r1, i1), = run([(0, ns)], rel, False)
        tag = (name, split, skip, rel)
        assert np.array_equal(T1, whole["transformation"]) and f1 == whole["fitness"] and r1 == whole["inlier_rmse"], tag
        assert not i1[2] and 0 <= i1[1] <= M_HOST
        if rel == 0.0:
            assert i1[1] == M_HOST and not i1[0], tag
        for sort in (False, True):
            for T, f, r, info in run(parts, rel, sort):
                assert np.array_equal(T, T1) and f == f1 and r == r1, tag + (sort,)
                assert np.array_equal(info, i1), tag + (sort, info.tolist(), i1.tolist())
