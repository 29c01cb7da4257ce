"""GPU parity of the strip-sweep loop kernel's error-minimiser sums, which reduce their nine fp64 accumulators over a wave
by one transposed tree (wave_sum_n, sfe_icp_common.h; the plan: sfe_wave_sum_plan.h, checked on the CPU by
tests/test_wave_sum_plan_host.py).  The brute-force kernel still reduces every sum by wave_sum, one after the other, so
pose, status and iteration count of every job are compared with it bit for bit; the well-posed jobs also with the oracle's
fp64-sum chain (status, iteration count, pose within 1e-6).

One list of jobs runs under both minimisers with 1, 3 and 30 iterations and on the shipped chain, on every build of the loop
kernel that takes the job's shape (the launcher's rule, as tests/test_gpu_icp_tiers.py selects it):
  * call "tiers": the jobs and 2 x CUs + 16 small fillers -> the one-wave build (at most 384 x 512 points), the four-wave
    build (at most 2048 x 2048), a 1024-thread build (the 4097-point job);
  * call "few": the jobs alone -> the four-wave build for at most 320 source points, a 1024-thread build for the rest;
  * call "one-size": tuning sw_tiers = 0 -> every job on a 1024-thread build;
  * call "brute": the brute-force kernel.
The routes are asserted, so a change of the launcher's rule fails loudly instead of quietly losing a build.

The jobs:
  * 1, 2, 63, 64, 65, 1023, 1024, 1025 and 4097 source points: the edges of lanes, waves, the 16 sum roles and the second
    pass over the roles;
  * clouds offset by about 1e3 m, so that the sums cancel;
  * a rank-deficient target of three points (the solve amplifies any change of the order of the sums): sources spread over
    the three, and sources that reach one of them only, where the last bits of the sums decide the rotation;
  * sources of which the distance filters keep one query of a wave only -- at lane 0, at lane 63 -- or one row of 16
    lanes only, alone in the job and beside full waves;
  * eight guesses on one pair;
  * a NaN source point (status and arrays with equal_nan; NaN payloads are not part of the contract).
The oracle is asked about the jobs whose result the order of the sums does not decide: not about the three-point target,
the jobs that keep one query or one row alone (one pair, or pairs on a line: rank-deficient as well) and the NaN jobs, where
its own order of summation gives other last bits and the solve amplifies them.

What the comparison can see: with the row totals of wave_sum_n added as (r0+r1)+(r2+r3), a library built aside, the
point-to-point cases with 3 and 30 iterations and the shipped chain fail on the jobs that reach one target point (all three
sizes, every build); no other job notices, and no point-to-plane case does -- its solve calls a system whose pivot has lost
ten digits singular instead of amplifying the noise (ICP_PIVOT_RTOL).  The ninth accumulator, which only that minimiser
fills, is therefore checked on the GPU against mistakes that change a sum beyond its last bits (a wrong partner, a wrong
lane for the total), and to the last bit by the CPU run of the plan."""
import contextlib
import functools
import os
from multiprocessing.pool import ThreadPool

import numpy as np
import pytest

import oracle
from sonar_slam_amd import _lib as L
from sonar_slam_amd import icp_config, synth
from sonar_slam_amd.pipeline import ScanMatchBatch

pytestmark = pytest.mark.gpu

TOL_TIGHT = 1e-6
ONE_SIZE = dict(sw_tiers=0, sw_multi=0, sw_tiny=0)
T0_SRC, T0_TGT, T1_SRC, T1_TGT, T1_FEW_SRC = 384, 512, 2048, 2048, 320   # the launcher's limits (sfe_icp_sweep.hip)
BIG = (L.ICP_ROUTE_Q, L.ICP_ROUTE_LDS, L.ICP_ROUTE_GLB, L.ICP_ROUTE_SPLIT)
SIZES = [(1, 400), (2, 400), (63, 400), (64, 400), (65, 400), (1023, 1500), (1024, 1500), (1025, 1500), (4097, 3000)]
FAR = np.float32(500.0)


def _keep_only(src, keep):
    """every source point outside `keep` moved far beyond the matcher's and the filter's distances"""
    out = src.copy()
    drop = np.ones(len(src), bool)
    drop[keep] = False
    out[drop] += FAR
    return out


@functools.lru_cache(maxsize=None)
def _jobs():
    """-> (sources, targets, jobs [(source, target)], guesses, names, oracle picks): built once, never changed"""
    rng = np.random.default_rng(2024)
    srcs, tgts, jobs, gs, names, picks = [], [], [], [], [], []

    def add(name, src, tgt, guess, ask_oracle, pair=None):
        if pair is None:
            srcs.append(np.ascontiguousarray(src, np.float32))
            tgts.append(np.ascontiguousarray(tgt, np.float32))
            pair = len(srcs) - 1
        if ask_oracle:
            picks.append(len(jobs))
        jobs.append((pair, pair))
        gs.append(np.asarray(guess, np.float32))
        names.append(name)
        return pair

    for k, (ns, nt) in enumerate(SIZES):
        s, t, g, _ = synth.scan_pair(seed=7000 + k, n_src=ns, n_tgt=nt)
        add("size %d" % ns, s, t, g, True)
    # offset by about 1e3 m: no rotation in the motion and little in the guess, so that the pose stays of the size of the
    # motion (a rotation about an origin 1e3 m away would put ~1e2 m into the float32 translation: 8e-6 per last bit)
    off = np.array([1000.0, -1000.0])
    To = synth.pose_matrix(off[0], off[1], 0.0)
    for k, (ns, nt) in enumerate([(300, 400), (1025, 1500)]):
        s, t, g, _ = synth.scan_pair(seed=7100 + k, n_src=ns, n_tgt=nt, motion=(0.8, -0.3, 0.0), guess_error=(0.3, -0.2, 0.01))
        g = To @ g.astype(np.float64) @ np.linalg.inv(To)
        add("offset %d" % ns, s.astype(np.float64) + off, t.astype(np.float64) + off, g, True)
    # three-point target
    for ns in (300, 1025):
        t = rng.uniform(-8, 8, (3, 2)).astype(np.float32)
        th = rng.uniform(-0.2, 0.2)
        R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        s = t[rng.integers(0, 3, ns)] @ R.T + rng.normal(0, 0.1, (ns, 2)) + rng.uniform(-0.3, 0.3, 2)
        add("three-point target %d" % ns, s, t, synth.pose_matrix(*rng.normal(0, [0.3, 0.3, 0.05])), False)
    # ... and a target with one point within the matcher's reach (the other two 40 m away): every kept pair has the same
    # neighbour, the point-to-point cross-covariance is zero in exact arithmetic and what the sums leave of it is rounding
    # noise that decides the rotation -- any other order of the adds, inside a row or over the rows, gives another pose
    for ns in (300, 1025, 4097):
        t = np.array([rng.uniform(-3, 3, 2), [40.0, rng.uniform(-3, 3)], [rng.uniform(-3, 3), 40.0]], np.float32)
        s = t[0] + rng.normal(0, 0.5, (ns, 2))
        add("one target point in reach %d" % ns, s, t, synth.pose_matrix(*rng.normal(0, [0.3, 0.3, 0.05])), False)
    # one query of a wave, one row of a wave: alone in the job ...
    s, t, g, _ = synth.scan_pair(seed=7200, n_src=64, n_tgt=400, outliers=0.0)
    for name, keep in (("lane 0 alone", [0]), ("lane 63 alone", [63]), ("row 2 alone", list(range(32, 48)))):
        add(name, _keep_only(s, keep), t, g, False)
    # ... and beside full waves: wave 0 keeps lane 0, wave 1 lane 63, wave 2 its row 1, the others everything (with 1100
    # queries the second pass over the roles keeps nothing, so that waves 0 .. 2 stay as they are)
    for ns in (384, 1100):
        s, t, g, _ = synth.scan_pair(seed=7300 + ns, n_src=ns, n_tgt=400 if ns <= T0_SRC else 1500, outliers=0.0)
        keep = [0, 64 + 63] + list(range(128 + 16, 128 + 32)) + list(range(192, min(ns, 1024)))
        add("sparse waves %d" % ns, _keep_only(s, keep), t, g, True)
    # eight guesses on one pair
    s, t, g, _ = synth.scan_pair(seed=7400, n_src=300, n_tgt=400)
    pair = None
    for k in range(8):
        gk = g.astype(np.float64) @ synth.pose_matrix(*rng.normal(0, [0.1, 0.1, 0.01]))
        pair = add("guess %d" % k, s, t, gk, True, pair)
    # a NaN source point
    for ns, nt, at in ((300, 400, 77), (1025, 1500, 1024)):
        s, t, g, _ = synth.scan_pair(seed=7500 + ns, n_src=ns, n_tgt=nt)
        s[at, 0] = np.nan
        add("NaN %d" % ns, s, t, g, False)
    # fillers (at the end, results unused): small jobs that keep the one-wave build live in the call "tiers"
    fs, ft, fg, _ = synth.scan_pair(seed=7600, n_src=24, n_tgt=24)
    srcs.append(fs)
    tgts.append(ft)
    return srcs, tgts, jobs, gs, names, picks, (len(srcs) - 1, fg)


def _run(ctx, p, srcs, tgts, jobs, gs, variant=0, **knobs):
    """one sfe_icp_jobs_dev call -> (T, status, iters, routes)"""
    b = ScanMatchBatch(ctx, p, srcs, tgts, jobs, gs)
    try:
        with ctx.tuning(**knobs):
            ctx._check(ctx.lib.sfe_icp_set_tuning(ctx.handle, variant))
            try:
                b.run()
            finally:
                ctx._check(ctx.lib.sfe_icp_set_tuning(ctx.handle, 0))
            routes = ctx.icp_routes(b.n)
            r = b.results()
    finally:
        b.free()
    return r["T"], r["status"], r["iters"], routes


def _same(a, b, n, names, what):
    for k, field in enumerate(("T", "status", "iters")):
        x, y = a[k][:n], b[k][:n]
        bad = np.flatnonzero((~((x == y) | ((x != x) & (y != y)))).reshape(n, -1).any(axis=1))
        assert bad.size == 0, (what, field, [names[j] for j in bad[:10]])


def _pose_diff(Ta, Tb):
    a, b = synth.pose_of(Ta), synth.pose_of(Tb)
    return max(abs(a[0] - b[0]), abs(a[1] - b[1]), abs(np.arctan2(np.sin(a[2] - b[2]), np.cos(a[2] - b[2]))))


@contextlib.contextmanager
def _kdtree():
    oracle.set_kdtree(True)
    try:
        yield
    finally:
        oracle.set_kdtree(False)


CHAINS = {"1": dict(max_iter=1, use_diff_checker=0), "3": dict(max_iter=3, use_diff_checker=0),
          "30": dict(max_iter=30, use_diff_checker=0), "shipped": {}}


@pytest.mark.parametrize("chain", list(CHAINS))
@pytest.mark.parametrize("minimizer", [0, 1])
def test_sums_on_every_build_equal_the_brute_force_kernel(ctx, minimizer, chain):
    p = icp_config.shipped_params(minimizer=minimizer, **CHAINS[chain])
    srcs, tgts, jobs, gs, names, picks, (fill_pair, fill_guess) = _jobs()
    n = len(jobs)
    shapes = [(len(srcs[a]), len(tgts[b])) for a, b in jobs]
    what = "minimizer %d, chain %s" % (minimizer, chain)

    brute = _run(ctx, p, srcs, tgts, jobs, gs, variant=4)
    assert (brute[3] == L.ICP_ROUTE_BRUTE).all()

    n_fill = 2 * ctx.n_cu + 16
    tiers = _run(ctx, p, srcs, tgts, jobs + [(fill_pair, fill_pair)] * n_fill, gs + [fill_guess] * n_fill, sw_tiny=0)
    for (s, t), r, name in zip(shapes, tiers[3], names):
        want = L.ICP_ROUTE_T0 if s <= T0_SRC and t <= T0_TGT else L.ICP_ROUTE_T1 if s <= T1_SRC and t <= T1_TGT else None
        assert r == want if want is not None else r in BIG, (what, name, r)
    assert (tiers[3][n:] == L.ICP_ROUTE_T0).all()
    _same(tiers, brute, n, names, (what, "tiers"))

    few = _run(ctx, p, srcs, tgts, jobs, gs, sw_tiny=0)
    for (s, t), r, name in zip(shapes, few[3], names):
        assert (r == L.ICP_ROUTE_T1) if s <= T1_FEW_SRC and t <= T1_TGT else r in BIG, (what, name, r)
    _same(few, brute, n, names, (what, "few"))

    one = _run(ctx, p, srcs, tgts, jobs, gs, **ONE_SIZE)
    assert all(r in BIG for r in one[3]), (what, np.unique(one[3]))
    _same(one, brute, n, names, (what, "one-size"))

    # the cases are what they are built for
    st = dict(zip(names, brute[1]))
    assert all(st["size %d" % s] == 0 for s, _ in SIZES[2:]) and st["offset 300"] == 0 and st["offset 1025"] == 0, (what, st)
    assert st["sparse waves 384"] == 0 and st["sparse waves 1100"] == 0 and all(st["guess %d" % k] == 0 for k in range(8)), (what, st)

    op = oracle.shipped_icp_params(precision=1, **p.as_dict())

    def ask(j):
        a, b = jobs[j]
        return oracle.icp(srcs[a], tgts[b], gs[j], op)

    with _kdtree(), ThreadPool(max(1, min(16, os.cpu_count() or 1))) as tp:
        ref = tp.map(ask, picks)
    for j, (sto, To, ito) in zip(picks, ref):
        info = (what, names[j])
        assert brute[1][j] == sto and brute[2][j] == ito, info + (int(brute[1][j]), sto, int(brute[2][j]), ito)
        if sto == 0:
            d = _pose_diff(tiers[0][j], To)
            assert d < TOL_TIGHT, info + (d,)
