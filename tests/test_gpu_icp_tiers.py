"""GPU parity of the ICP launcher's small-job tiers at the batch sizes that select them.

The strip-sweep launcher (sfe_icp_sweep.hip) sends a job to the one-wave build of the loop kernel only when the call
brings at least 2 x CUs such jobs, and lets the four-wave build take jobs of more than 320 source points only when the
call brings at least 2 x CUs small jobs.  The batches here are sized from the context's CU count (2 x n_cu + a margin),
and every test asserts the route each job took (sfe_icp_last_routes), so a change of the heuristic fails loudly instead
of quietly losing coverage.  References: the oracle in fp64-sum mode (status, iteration count, pose within 1e-6), the
same batch with every job on the 1024-thread build (bit for bit: every build adds the error minimiser's sums in the
order of a 1024-thread workgroup) and the brute-force kernel (bit for bit)."""
import contextlib
import os
from multiprocessing.pool import ThreadPool

import numpy as np
import pytest

import oracle
from sonar_slam_amd import _lib as L
from sonar_slam_amd import icp_config, pcl, synth
from sonar_slam_amd._lib import IcpParams
from sonar_slam_amd.pipeline import ScanMatchBatch

pytestmark = pytest.mark.gpu

TOL_TIGHT = 1e-6
ONE_SIZE = dict(sw_tiers=0, sw_multi=0, sw_tiny=0)
# the launcher's limits (sfe_icp_sweep.h, sfe_icp_sweep.hip)
TINY_MAX, TINY_PAIRS_SHORT, TINY_PAIRS_LONG, REC_MIN_ITER = 512, 400000, 120000, 12
T0_SRC, T0_TGT, T1_SRC, T1_TGT, T1_FEW_SRC = 384, 512, 2048, 2048, 320

P2P_REC = dict(max_iter=30, use_diff_checker=0)                       # fixed count: the clearance-record build
P2PLANE_REC = dict(minimizer=1, max_iter=30, use_diff_checker=0)


def _pose_diff(Ta, Tb):
    a, b = synth.pose_of(Ta), synth.pose_of(Tb)
    return max(abs(a[0] - b[0]), abs(a[1] - b[1]), abs(np.arctan2(np.sin(a[2] - b[2]), np.cos(a[2] - b[2]))))


def _with_variant(ctx, variant, fn):
    ctx._check(ctx.lib.sfe_icp_set_tuning(ctx.handle, variant))
    try:
        return fn()
    finally:
        ctx._check(ctx.lib.sfe_icp_set_tuning(ctx.handle, 0))


def _small_routes(sizes, p, n_cu, tiers=True, tiny=True):
    """the launcher's rule for jobs of at most 2048 x 2048 points: ROUTE_TINY / _T0 / _T1, or None (a 1024-thread
    build) for each (n_src, n_tgt) of one call"""
    short = p.use_diff_checker or p.max_iter < REC_MIN_ITER
    pairs = TINY_PAIRS_SHORT if short else TINY_PAIRS_LONG
    fit0 = [tiers and s <= T0_SRC and t <= T0_TGT for s, t in sizes]
    fit1 = [tiers and not f0 and s <= T1_SRC and t <= T1_TGT for f0, (s, t) in zip(fit0, sizes)]
    use_t0 = sum(fit0) >= 2 * n_cu
    few_small = sum(fit0) + sum(fit1) < 2 * n_cu
    out = []
    for (s, t), f0 in zip(sizes, fit0):
        if tiny and s <= TINY_MAX and t <= TINY_MAX and s * t <= pairs:
            out.append(L.ICP_ROUTE_TINY)
        elif use_t0 and f0:
            out.append(L.ICP_ROUTE_T0)
        elif tiers and s <= T1_SRC and t <= T1_TGT and (not few_small or s <= T1_FEW_SRC):
            out.append(L.ICP_ROUTE_T1)
        else:
            out.append(None)
    return out


def _tile(pairs, n, rng, base=0):
    """n jobs over the distinct (source, target, guess) pairs, one after the other, each guess perturbed a little (as
    tools/bench_legs.py real_size does) -> (jobs, guesses); job k < len(pairs) is pair base + k"""
    d = len(pairs)
    jobs = [(base + j % d, base + j % d) for j in range(n)]
    gs = [(pairs[j % d][2].astype(np.float64) @ synth.pose_matrix(*rng.normal(0, [0.05, 0.05, 0.005]))).astype(np.float32)
          for j in range(n)]
    return jobs, gs


def _run(ctx, p, srcs, tgts, jobs, gs, variant=0, **knobs):
    """one sfe_icp_jobs_dev call -> (T, status, iters, routes)"""
    b = ScanMatchBatch(ctx, p, srcs, tgts, jobs, gs)
    try:
        with ctx.tuning(**knobs):
            _with_variant(ctx, variant, b.run)
            routes = ctx.icp_routes(b.n)
            r = b.results()
    finally:
        b.free()
    return r["T"], r["status"], r["iters"], routes


def _same(a, b, what):
    for k, name in enumerate(("T", "status", "iters")):
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, name, np.flatnonzero(
            (a[k] != b[k]).reshape(len(a[1]), -1).any(axis=1))[:10])


@contextlib.contextmanager
def _kdtree():
    """the oracle's exact kd-tree behind its searches (same neighbours; test_oracle_pipeline pins it to brute force)"""
    oracle.set_kdtree(True)
    try:
        yield
    finally:
        oracle.set_kdtree(False)


def _check_oracle(p, picks, srcs, tgts, jobs, gs, got, what):
    """the picked jobs against the oracle's fp64-sum chain: same status and iteration count, pose within 1e-6"""
    op = oracle.shipped_icp_params(precision=1, **p.as_dict())

    def one(j):
        a, b = jobs[j]
        return oracle.icp(srcs[a], tgts[b], gs[j], op)

    with _kdtree(), ThreadPool(max(1, min(16, os.cpu_count() or 1))) as tp:
        ref = tp.map(one, picks)
    for j, (st, To, ito) in zip(picks, ref):
        info = (what, j, len(srcs[jobs[j][0]]), len(tgts[jobs[j][1]]))
        assert got[1][j] == st and got[2][j] == ito, info + (int(got[1][j]), st, int(got[2][j]), ito)
        if st == 0:
            assert _pose_diff(got[0][j], To) < TOL_TIGHT, info + (_pose_diff(got[0][j], To),)


def _pairs(sizes, seed0):
    return [synth.scan_pair(seed=seed0 + i, n_src=a, n_tgt=b) for i, (a, b) in enumerate(sizes)]


@pytest.mark.parametrize("chain", ["shipped", "p2p30", "p2plane30", "trim03"])
def test_four_wave_tier_with_more_than_eight_sum_roles(ctx, chain):
    """Jobs of 321..2048 source points on targets of 513..2048 in a call of 2 x CUs + 64 such jobs: all on the
    four-wave build, most of them with more than 512 queries, i.e. more than eight of the sixteen sum roles of a
    1024-thread workgroup (each of the four waves plays four of them).  The shipped chain runs the build without
    clearance records, the 30-iteration chains the one with them."""
    over = {"shipped": {}, "p2p30": P2P_REC, "p2plane30": P2PLANE_REC,
            "trim03": dict(trim_ratio=0.3, use_max_dist_filter=1, max_dist_filter=1.0)}[chain]
    p = icp_config.shipped_params(**over)
    rng = np.random.default_rng(31)
    edges = [448, 512, 513, 520, 576, 577, 1023, 1024, 1025, 2047, 2048]
    sizes = [(s, int(t)) for s, t in zip(edges, rng.integers(513, 2049, len(edges)))]
    sizes += [(2048, 2048), (513, 2048), (1024, 513)]
    sizes += [(int(a), int(b)) for a, b in zip(rng.integers(321, 2049, 50), rng.integers(513, 2049, 50))]
    pairs = _pairs(sizes, 3100)
    srcs, tgts = [q[0] for q in pairs], [q[1] for q in pairs]
    n = 2 * ctx.n_cu + 64
    jobs, gs = _tile(pairs, n, rng)
    got = _run(ctx, p, srcs, tgts, jobs, gs)
    shapes = [(len(srcs[a]), len(tgts[b])) for a, b in jobs]
    assert all(r == L.ICP_ROUTE_T1 for r in got[3]), np.unique(got[3])
    assert list(got[3]) == _small_routes(shapes, p, ctx.n_cu)
    assert sum(s > 512 for s, _ in shapes) >= 100
    _check_oracle(p, list(range(len(pairs))), srcs, tgts, jobs, gs, got, chain)
    assert (got[1][:len(pairs)] == 0).sum() >= len(pairs) // 2      # mostly converged: the poses are compared
    _same(got, _run(ctx, p, srcs, tgts, jobs, gs, **ONE_SIZE), (chain, "one-size"))


@pytest.mark.parametrize("variant", ["no-tiny-kernel", "long-chain"])
def test_one_wave_tier(ctx, variant):
    """2 x CUs + 64 jobs of at most 384 x 512 points: the one-wave build.  Without the tiny kernel (tuning sw_tiny = 0)
    on the shipped chain (the build without clearance records); with default tuning on a 30-iteration chain with
    shapes above the tiny kernel's pair limit for long chains (the build with them).  The jobs just past the tier's
    limits, (385, 512) and (384, 513), go to the four-wave build."""
    rng = np.random.default_rng(32 if variant == "long-chain" else 33)
    if variant == "long-chain":
        p, knobs = icp_config.shipped_params(**P2P_REC), {}
        src_n = rng.integers(300, 385, 45)
        sizes = [(int(a), int(rng.integers(TINY_PAIRS_LONG // a + 1, 513))) for a in src_n]
    else:
        p, knobs = icp_config.shipped_params(), dict(sw_tiny=0)
        sizes = [(int(a), int(b)) for a, b in zip(rng.integers(40, 385, 45), rng.integers(40, 513, 45))]
        sizes += [(1, 512), (384, 1), (1, 1)]
    sizes += [(384, 512), (385, 512), (384, 513), (384, 384)]
    pairs = _pairs(sizes, 3300)
    srcs, tgts = [q[0] for q in pairs], [q[1] for q in pairs]
    n = 2 * ctx.n_cu + 64
    jobs, gs = _tile(pairs, n, rng)
    got = _run(ctx, p, srcs, tgts, jobs, gs, **knobs)
    shapes = [(len(srcs[a]), len(tgts[b])) for a, b in jobs]
    want = [L.ICP_ROUTE_T0 if s <= T0_SRC and t <= T0_TGT else L.ICP_ROUTE_T1 for s, t in shapes]
    assert list(got[3]) == want
    assert list(got[3]) == _small_routes(shapes, p, ctx.n_cu, tiny=not knobs)
    assert sum(r == L.ICP_ROUTE_T0 for r in got[3]) >= 2 * ctx.n_cu
    _same(got, _run(ctx, p, srcs, tgts, jobs, gs, **ONE_SIZE), (variant, "one-size"))
    _check_oracle(p, list(range(len(pairs))), srcs, tgts, jobs, gs, got, variant)


@pytest.mark.parametrize("chain", ["shipped", "short-fixed", "long-fixed"])
def test_tiny_kernel_limits(ctx, chain):
    """The exhaustive one-wave kernel takes clouds of at most 512 points and at most 400 000 (chains with the
    differential checker or fewer than 12 iterations) or 120 000 (longer fixed chains) point pairs.  Two clouds of 512
    points make 262 144 pairs, so the short limit is only met from below: its chains must keep the largest jobs.
    The rest of the call (2 x CUs + 64 jobs) keeps the one-wave sweep tier live for the jobs just past a limit."""
    over = {"shipped": {}, "short-fixed": dict(max_iter=REC_MIN_ITER - 1, use_diff_checker=0),
            "long-fixed": dict(max_iter=REC_MIN_ITER, use_diff_checker=0)}[chain]
    p = icp_config.shipped_params(**over)
    rng = np.random.default_rng(34)
    sizes = [(512, 512), (513, 512), (512, 513), (513, 300), (300, 513), (384, 512), (512, 200), (200, 512)]
    sizes += [(300, 400), (300, 401), (400, 300), (401, 300), (240, 500), (241, 500), (346, 346), (347, 346)]
    sizes += [(int(a), int(b)) for a, b in zip(rng.integers(100, 385, 32), rng.integers(100, 513, 32))]
    sizes.sort(key=lambda st: not (st[0] <= T0_SRC and st[1] <= T0_TGT))   # the one-wave tier's shapes first ...
    n0 = sum(s <= T0_SRC and t <= T0_TGT for s, t in sizes)
    pairs = _pairs(sizes, 3400)
    srcs, tgts = [q[0] for q in pairs], [q[1] for q in pairs]
    n = 2 * ctx.n_cu + 64
    jobs, gs = _tile(pairs[:n0], 2 * ctx.n_cu, rng)                       # ... 2 x CUs of them in the call
    j1, g1 = _tile(pairs[n0:], n - 2 * ctx.n_cu, rng, base=n0)
    jobs += j1
    gs += g1
    got = _run(ctx, p, srcs, tgts, jobs, gs)
    shapes = [(len(srcs[a]), len(tgts[b])) for a, b in jobs]
    want = _small_routes(shapes, p, ctx.n_cu)
    assert list(got[3]) == want
    limit = TINY_PAIRS_LONG if chain == "long-fixed" else TINY_PAIRS_SHORT
    for (s, t), r in zip(shapes, got[3]):
        assert (r == L.ICP_ROUTE_TINY) == (s <= TINY_MAX and t <= TINY_MAX and s * t <= limit), (s, t, r)
    assert {L.ICP_ROUTE_TINY, L.ICP_ROUTE_T1} <= set(got[3])
    if chain == "long-fixed":
        assert L.ICP_ROUTE_T0 in set(got[3])
    _same(got, _run(ctx, p, srcs, tgts, jobs, gs, **ONE_SIZE), (chain, "one-size"))
    picks = list(range(n0)) + list(range(2 * ctx.n_cu, 2 * ctx.n_cu + len(pairs) - n0))
    _check_oracle(p, picks, srcs, tgts, jobs, gs, got, chain)


BIG_ROUTES = [L.ICP_ROUTE_Q, L.ICP_ROUTE_Q, L.ICP_ROUTE_LDS, L.ICP_ROUTE_LDS, L.ICP_ROUTE_GLB, L.ICP_ROUTE_GLB]


def _every_class_batch(ctx):
    """2 x CUs + 64 small jobs (tiny, one-wave and four-wave shapes) and the six 1024-thread jobs of BIG_ROUTES behind
    them -> (srcs, tgts, jobs, guesses, n = the number of small jobs, n0 = the number of tiny and one-wave pairs, which
    come first among the distinct pairs)"""
    rng = np.random.default_rng(35)
    sizes = [(int(a), int(b)) for a, b in zip(rng.integers(60, 300, 12), rng.integers(60, 300, 12))]      # tiny
    sizes += [(int(a), int(b)) for a, b in zip(rng.integers(330, 385, 12), rng.integers(400, 513, 12))]   # one wave
    n0 = len(sizes)
    sizes += [(int(a), int(b)) for a, b in zip(rng.integers(600, 2049, 8), rng.integers(513, 2049, 8))]   # four waves
    n_small = len(sizes)
    big = [(3000, 3000), (2500, 6000), (18000, 8192), (16500, 8000), (2000, 9000), (4000, 12000)]
    pairs = _pairs(sizes + big, 3500)
    srcs, tgts = [q[0] for q in pairs], [q[1] for q in pairs]
    n = 2 * ctx.n_cu + 64
    jobs, gs = _tile(pairs[:n0], 2 * ctx.n_cu, rng)
    j1, g1 = _tile(pairs[n0:n_small], n - 2 * ctx.n_cu, rng, base=n0)
    jobs += j1
    gs += g1 + [q[2] for q in pairs[n_small:]]
    jobs += [(n_small + i, n_small + i) for i in range(len(big))]
    return srcs, tgts, jobs, gs, n, n0


def test_every_job_class_in_one_call(ctx):
    """Tiny, one-wave, four-wave and 1024-thread jobs (queries in LDS, target in LDS with the per-query results in HBM,
    target in HBM) side by side in one call that holds 2 x CUs small jobs, so that both small tiers are live."""
    p = icp_config.shipped_params(**P2P_REC)
    srcs, tgts, jobs, gs, n, n0 = _every_class_batch(ctx)
    got = _run(ctx, p, srcs, tgts, jobs, gs)
    r = list(got[3])
    shapes = [(len(srcs[a]), len(tgts[b])) for a, b in jobs]
    assert r[:n] == _small_routes(shapes, p, ctx.n_cu)[:n]
    assert r[n:] == BIG_ROUTES
    for route in (L.ICP_ROUTE_TINY, L.ICP_ROUTE_T0, L.ICP_ROUTE_T1):
        assert r[:n].count(route) >= 8, route
    _same(got, _run(ctx, p, srcs, tgts, jobs, gs, **ONE_SIZE), "one-size")
    picks = [r.index(route) for route in (L.ICP_ROUTE_TINY, L.ICP_ROUTE_T0, L.ICP_ROUTE_T1)]
    picks = sorted(set(picks + [n0 - 1, 2 * ctx.n_cu, n - 1] + list(range(n, len(jobs)))))
    _check_oracle(p, picks, srcs, tgts, jobs, gs, got, "every class")


def _degenerate_job(rng, kind, ns):
    """(source, target) of one awkward job: kind 0 = a target of 1..7 points (duplicates, points on lines of equal x),
    1 = an ordinary cloud with NaN and far-outlier source points, 2 = a source far from its target (no pair survives)"""
    if kind == 1:
        nt = int(rng.integers(40, 513)) if ns <= T0_SRC else int(rng.integers(513, 2049))
        tgt = rng.uniform(-8, 8, (nt, 2)).astype(np.float32)
    else:
        nt = int(rng.integers(1, 8))
        tgt = rng.uniform(-8, 8, (nt, 2)).astype(np.float32)
        if rng.random() < 0.5:
            tgt[:, 0] = np.round(tgt[:, 0] * 2) / 2
        if nt > 3 and rng.random() < 0.6:
            tgt[nt // 2:] = tgt[:nt - nt // 2]
    th = rng.uniform(-0.2, 0.2)
    R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    src = (tgt[rng.integers(0, len(tgt), ns)] @ R.T + rng.normal(0, 0.1, (ns, 2)) + rng.uniform(-0.3, 0.3, 2)).astype(np.float32)
    if kind == 1:
        src[rng.integers(0, ns, 3)] += 100.0
        src[rng.integers(0, ns), int(rng.integers(0, 2))] = np.nan
    elif kind == 2:
        src += np.float32(500.0)
    return src, tgt


def test_degenerate_jobs_on_the_small_tiers(ctx):
    """Targets of 1..7 points (rank-deficient systems whose pose the last bit of an fp64 sum decides, with 150..384 and
    with 513..2048 source points), NaN and far-outlier sources, and jobs that keep no pair, on the one-wave and four-wave
    builds (tuning sw_tiny = 0; 2 x CUs + 16 one-wave jobs and 112 four-wave ones per call), under eight parameter sets
    drawn like test_gpu_icp's fuzz: bit-identical to the 1024-thread build and to the brute-force kernel."""
    rng = np.random.default_rng(36)
    n0, n1 = 2 * ctx.n_cu + 16, 112
    n_fail = n_ok = 0
    for case in range(8):
        srcs, tgts = [], []
        kinds = [(0, 0, 1, 2)[j % 4] for j in range(n0)] + [(0, 0, 0, 1, 2)[j % 5] for j in range(n1)]
        for j, kind in enumerate(kinds):
            ns = int(rng.integers(150, T0_SRC + 1)) if j < n0 else int(rng.integers(513, 2049))
            s, t = _degenerate_job(rng, kind, ns)
            srcs.append(s)
            tgts.append(t)
        gs = [synth.pose_matrix(*rng.normal(0, [0.3, 0.3, 0.05])).astype(np.float32) for _ in srcs]
        p = IcpParams(matcher_max_dist=float(rng.choice([0.5, 3.0, 10.0])), use_max_dist_filter=int(rng.integers(0, 2)),
                      max_dist_filter=float(rng.choice([0.3, 3.0, 20.0])), use_trimmed_filter=int(rng.integers(0, 2)),
                      trim_ratio=float(rng.choice([0.3, 0.8, 1.0])), minimizer=int(case % 4 == 3),
                      max_iter=int(rng.integers(1, 15)) if case % 2 else 30, use_diff_checker=int(rng.integers(0, 2)) if case % 2 else 0,
                      min_diff_rot=0.001, min_diff_trans=0.01, smooth_len=int(rng.integers(1, 4)),
                      normals_knn=int(rng.integers(2, 17)))
        jobs = [(j, j) for j in range(len(srcs))]
        got = _run(ctx, p, srcs, tgts, jobs, gs, sw_tiny=0)
        assert list(got[3]) == [L.ICP_ROUTE_T0] * n0 + [L.ICP_ROUTE_T1] * n1, case
        _same(got, _run(ctx, p, srcs, tgts, jobs, gs, **ONE_SIZE), (case, "one-size", p.as_dict()))
        brute = _run(ctx, p, srcs, tgts, jobs, gs, variant=4)
        assert (brute[3] == L.ICP_ROUTE_BRUTE).all()
        _same(got, brute, (case, "brute force", p.as_dict()))
        failed = got[1] != 0
        assert failed[np.array(kinds) == 2].all(), case                 # no pair kept: a failure status ...
        for j in np.flatnonzero(failed):
            assert np.array_equal(got[0][j], gs[j]), (case, j)          # ... and the guess comes back
        n_fail += int(failed.sum())
        n_ok += int((~failed).sum())
    assert n_fail > 0 and n_ok > 0


def test_routes_report_the_last_call(ctx):
    """sfe_icp_last_routes answers for the last ICP call on the context and refuses a job count that is not its own"""
    src, tgt, guess, _ = synth.scan_pair(seed=37, n_src=300, n_tgt=300)
    icp = pcl.ICP(ctx)
    icp.setParams(icp_config.shipped_params())
    icp.compute_pairs([src, src[:200]], [tgt, tgt], [guess, guess])
    assert list(ctx.icp_routes(2)) == [L.ICP_ROUTE_TINY] * 2
    with pytest.raises(L.SonarFEError):
        ctx.icp_routes(3)
    with ctx.tuning(sw_tiny=0):
        icp.compute_pairs([src], [tgt], [guess])
    assert list(ctx.icp_routes(1)) == [L.ICP_ROUTE_T1]     # one small job: the four-wave build (at most 320 queries)
    _with_variant(ctx, 4, lambda: icp.compute_pairs([src], [tgt], [guess]))
    assert list(ctx.icp_routes(1)) == [L.ICP_ROUTE_BRUTE]
    assert ctx.n_cu >= 1
