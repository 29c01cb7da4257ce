"""GPU parity of the ICP kernels' strip-wise sorts (strip_sort_lds, sfe_icp_sweep.h).

The target preparation sorts (strip, x, index) keys of the target, the loop kernel those of the queries under the guess:
both count the keys per strip, scatter them into the strips' segments and sort every segment inside one wave; a strip
of more than SEG_MAX keys sends the whole key set through the full bitonic network instead.  The sorted order is fully
determined (the index is part of the key), so every result must stay what it was.  The tests drive the public entry
points (ScanMatchBatch) with the tiny exhaustive kernel switched off (tuning sw_tiny = 0: it does not sort), on the
builds a call of a few jobs selects (256 threads for at most 320 queries and targets of at most 2048 points, 1024
threads otherwise), with every job on the 1024-thread builds (sw_tiers = 0) and, once, on the one-wave build.
References, as in test_gpu_icp_tiers: the brute-force kernel (bit for bit) and the oracle in fp64-sum mode (status and
iteration count equal, pose within 1e-6).  Clouds on one line (a singular point-to-plane system, whose pose the last
bit of a sum decides) are held against the brute-force kernel alone."""
import contextlib
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
SEG_MAX = 1024                     # SW_SEG_MAX (sfe_icp_sweep.h)
PAD = 68                           # SW_PAD
NO_TINY = dict(sw_tiny=0)
ONE_SIZE = dict(sw_tiers=0, sw_multi=0, sw_tiny=0)
CHAINS = {"p2p": {}, "p2plane": dict(minimizer=1, max_iter=30, use_diff_checker=0)}


def _pose_diff(Ta, Tb):
    a, b = synth.pose_of(Ta), synth.pose_of(Tb)
    return max(abs(a[0] - b[0]), abs(a[1] - b[1]), abs(np.arctan2(np.sin(a[2] - b[2]), np.cos(a[2] - b[2]))))


def _run(ctx, p, srcs, tgts, jobs, gs, variant=0, **knobs):
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


def _same(a, b, what):
    for k, name in enumerate(("T", "status", "iters")):
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, name, np.flatnonzero(
            (a[k] != b[k]).reshape(len(a[1]), -1).any(axis=1))[:10])


@contextlib.contextmanager
def _kdtree():
    oracle.set_kdtree(True)
    try:
        yield
    finally:
        oracle.set_kdtree(False)


def _check_oracle(p, picks, srcs, tgts, jobs, gs, got, what):
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


def _check(ctx, chain, srcs, tgts, gs, what, with_oracle=True, jobs=None, want_routes=None):
    """the jobs on the builds the call selects and on the 1024-thread builds: both bit for bit the brute-force kernel,
    the first against the oracle; -> the results"""
    p = icp_config.shipped_params(**CHAINS[chain])
    jobs = jobs if jobs is not None else [(j, j) for j in range(len(srcs))]
    got = _run(ctx, p, srcs, tgts, jobs, gs, **NO_TINY)
    assert not set(got[3]) & {L.ICP_ROUTE_TINY, L.ICP_ROUTE_BRUTE}, np.unique(got[3])
    if want_routes is not None:
        assert list(got[3]) == want_routes, list(got[3])
    brute = _run(ctx, p, srcs, tgts, jobs, gs, variant=4)
    assert (brute[3] == L.ICP_ROUTE_BRUTE).all()
    _same(got, brute, (what, chain, "brute force"))
    one = _run(ctx, p, srcs, tgts, jobs, gs, **ONE_SIZE)
    assert not set(one[3]) & {L.ICP_ROUTE_TINY, L.ICP_ROUTE_T0, L.ICP_ROUTE_T1, L.ICP_ROUTE_BRUTE}, np.unique(one[3])
    _same(one, brute, (what, chain, "1024 threads against brute force"))
    if with_oracle:
        _check_oracle(p, list(range(len(jobs))), srcs, tgts, jobs, gs, got, (what, chain))
    return got


def _guess(rng):
    return synth.pose_matrix(*rng.normal(0, [0.2, 0.2, 0.03])).astype(np.float32)


def _moved(rng, tgt, ns, noise=0.03):
    """ns source points: target points moved by a small pose, with noise"""
    T = np.linalg.inv(synth.pose_matrix(0.3, -0.2, 0.04))
    pts = tgt[rng.integers(0, len(tgt), ns)].astype(np.float64) + rng.normal(0, noise, (ns, 2))
    return (pts @ T[:2, :2].T + T[:2, 2]).astype(np.float32)


EDGES = [1, 2, 3, 63, 64, 65, 127, 129, 511, 513, 2047, 2048, 5000]


@pytest.mark.parametrize("chain", list(CHAINS))
def test_sizes_at_the_edges_of_the_network(ctx, chain):
    """Clouds of 1 .. 5000 points, n x n for every edge size and a few mixed pairs: segments of 0, 1, 2 keys, one short of /
    at / one past a power of two, the 256-thread preparation at its capacity (2048) and the 1024-thread one."""
    sizes = [(n, n) for n in EDGES] + [(2048, 129), (129, 2048), (5000, 513), (65, 5000)]
    pairs = [synth.scan_pair(seed=4100 + i, n_src=a, n_tgt=b) for i, (a, b) in enumerate(sizes)]
    srcs, tgts, gs = [q[0] for q in pairs], [q[1] for q in pairs], [q[2] for q in pairs]
    got = _check(ctx, chain, srcs, tgts, gs, "edges")
    assert {L.ICP_ROUTE_T1, L.ICP_ROUTE_Q} <= set(got[3]), np.unique(got[3])
    assert (got[1][8:] == 0).all()                          # the clouds of 511 points and more converge


@pytest.mark.parametrize("chain", list(CHAINS))
def test_one_wave_build(ctx, chain):
    """2 x CUs + 16 jobs of at most 384 x 512 points in one call: the one-wave builds of both kernels (one wave sorts
    every segment, no second wave to share them with)"""
    rng = np.random.default_rng(42)
    sizes = [(n, n) for n in EDGES[:8]] + [(384, 511), (383, 512), (129, 65), (3, 384)]
    pairs = [synth.scan_pair(seed=4200 + i, n_src=a, n_tgt=b) for i, (a, b) in enumerate(sizes)]
    srcs, tgts = [q[0] for q in pairs], [q[1] for q in pairs]
    n = 2 * ctx.n_cu + 16
    jobs = [(j % len(pairs), j % len(pairs)) for j in range(n)]
    gs = [(pairs[j % len(pairs)][2].astype(np.float64) @ synth.pose_matrix(*rng.normal(0, [0.05, 0.05, 0.005]))).astype(np.float32)
          if j >= len(pairs) else pairs[j][2] for j in range(n)]
    p = icp_config.shipped_params(**CHAINS[chain])
    got = _run(ctx, p, srcs, tgts, jobs, gs, **NO_TINY)
    assert list(got[3]) == [L.ICP_ROUTE_T0] * n
    brute = _run(ctx, p, srcs, tgts, jobs, gs, variant=4)
    _same(got, brute, (chain, "brute force"))
    _check_oracle(p, list(range(len(pairs))), srcs, tgts, jobs, gs, got, ("one wave", chain))


def _two_clusters(rng, n):
    """n points in two blobs 40 m apart in y: nearly every strip in between is empty"""
    c = np.where(rng.random(n) < 0.5, -20.0, 20.0)
    return np.c_[rng.uniform(-6, 6, n), c + rng.uniform(-0.8, 0.8, n) + 0.3 * np.sin(rng.uniform(0, 6, n))].astype(np.float32)


def _on_a_line(rng, n, y=1.5):
    return np.c_[np.sort(rng.uniform(-20, 20, n)), np.full(n, y)].astype(np.float32)


@pytest.mark.parametrize("chain", list(CHAINS))
def test_empty_strips(ctx, chain):
    """two y-clusters far apart, in a 256-thread and a 1024-thread job (20 and 41 strips, two or three of them filled)"""
    rng = np.random.default_rng(43)
    tgts = [_two_clusters(rng, 2000), _two_clusters(rng, 4000)]
    srcs = [_moved(rng, tgts[0], 300), _moved(rng, tgts[1], 3500)]
    gs = [_guess(rng) for _ in srcs]
    _check(ctx, chain, srcs, tgts, gs, "two clusters", want_routes=[L.ICP_ROUTE_T1, L.ICP_ROUTE_Q])


@pytest.mark.parametrize("chain", list(CHAINS))
def test_one_strip_below_at_and_above_the_cap(ctx, chain):
    """Every point of the target at one y: one strip holds them all (the table's inv_g is 0, so every query lands in it
    as well).  600 points: a single segment far below the cap; SEG_MAX - 1 and SEG_MAX: the largest segments one wave
    sorts; SEG_MAX + 1: both kernels take the full network.  Source clouds of the same sizes, so the query sort meets
    the same three counts."""
    rng = np.random.default_rng(44)
    base = _on_a_line(rng, SEG_MAX + 1)
    ns_ = [600, SEG_MAX - 1, SEG_MAX, SEG_MAX + 1]
    tgts = [np.ascontiguousarray(base[:n]) for n in ns_]
    srcs = [_moved(rng, t, len(t)) for t in tgts]
    gs = [_guess(rng) for _ in srcs]
    got = _check(ctx, chain, srcs, tgts, gs, "one strip", with_oracle=False)
    # the same cloud under the three counts around the cap: each of them was held against the exhaustive kernel above;
    # the runs below and above the cap also agree on what they are (no failure status hides a difference)
    assert len(set(got[1][1:])) == 1, got[1]


@pytest.mark.parametrize("chain", list(CHAINS))
def test_duplicate_points(ctx, chain):
    """repeated (x, y) points and x values repeated inside a strip, in both clouds: equal (strip, x) keys differ by
    their index alone, and the k-NN ties of the normals are broken through the sorted order"""
    rng = np.random.default_rng(45)
    src0, tgt0, g, _ = synth.scan_pair(seed=4500, n_src=1500, n_tgt=1500)
    tgt = tgt0.copy()
    tgt[:, 0] = np.round(tgt[:, 0] * 4) / 4                 # x on a 0.25 m grid: many equal x inside a strip
    tgt[700:1400] = tgt[:700]                               # every second point twice
    src = src0.copy()
    src[:, 0] = np.round(src[:, 0] * 4) / 4
    src[750:1500] = src[:750]
    t2 = np.ascontiguousarray(tgt[rng.permutation(1500)][:1100])
    s2 = np.ascontiguousarray(src[rng.permutation(1500)][:300])
    _check(ctx, chain, [src, s2], [tgt, t2], [g, g], "duplicates", want_routes=[L.ICP_ROUTE_Q, L.ICP_ROUTE_T1])


@pytest.mark.parametrize("chain", list(CHAINS))
def test_nan_points(ctx, chain):
    """NaN coordinates in source and target, placed as test_gpu_icp's fuzz places them: a NaN y lands in strip 0, a NaN
    x sorts behind every finite x of its strip"""
    rng = np.random.default_rng(46)
    srcs, tgts, gs = [], [], []
    for i, (ns, nt) in enumerate([(1500, 1500), (300, 1200), (2500, 600)]):
        s, t, g, _ = synth.scan_pair(seed=4600 + i, n_src=ns, n_tgt=nt)
        s, t = s.copy(), t.copy()
        s[rng.integers(0, ns, 3), 0] = np.nan
        s[rng.integers(0, ns, 3), 1] = np.nan
        if i != 1:
            t[rng.integers(0, nt, 3), 0] = np.nan
            t[rng.integers(0, nt, 3), 1] = np.nan
        srcs.append(s)
        tgts.append(t)
        gs.append(g)
    # (the oracle's kd-tree is pinned to brute force on finite targets: the jobs with NaN targets are held against
    # the brute-force kernel, the one with a clean target against the oracle too)
    _check(ctx, chain, srcs, tgts, gs, "nan", with_oracle=False)
    _check(ctx, chain, srcs[1:2], tgts[1:2], gs[1:2], "nan source")


@pytest.mark.parametrize("chain", list(CHAINS))
def test_source_larger_than_one_sort_chunk(ctx, chain):
    """The queries are sorted in chunks of the largest power of two of keys that fits the LDS behind the control block:
    (8 (n_tgt + SW_PAD) + 6 n_src) / 8 for a job whose results live in LDS.  700 queries on a 60-point target make
    that 653 -> chunks of 512, on the 1024-thread build; 300 queries on a 100-point target 393 -> chunks of 256, on
    the 256-thread build (which takes at most 320 queries when the call holds few small jobs).  Two chunks each, the
    smallest shapes that have them: every chunk is ordered on its own."""

    def chunk(ns, nt):
        c = 1
        while 2 * c <= (8 * (nt + PAD) + 6 * ((ns + 3) & ~3)) // 8:
            c *= 2
        return c

    assert chunk(700, 60) == 512 and chunk(300, 100) == 256
    s0, t0, g0, _ = synth.scan_pair(seed=4700, n_src=700, n_tgt=60)
    s1, t1, g1, _ = synth.scan_pair(seed=4701, n_src=300, n_tgt=100)
    _check(ctx, chain, [s0], [t0], [g0], "chunks of 512", want_routes=[L.ICP_ROUTE_Q])
    _check(ctx, chain, [s1], [t1], [g1], "chunks of 256", want_routes=[L.ICP_ROUTE_T1])


@pytest.mark.parametrize("chain", list(CHAINS))
def test_many_guesses_on_one_target(ctx, chain):
    """one target, eight guesses: one preparation (one sorted target, one set of normals) serves eight jobs"""
    rng = np.random.default_rng(48)
    src, tgt, g, _ = synth.scan_pair(seed=4800, n_src=1800, n_tgt=2300)
    gs = [g] + [(g.astype(np.float64) @ synth.pose_matrix(*rng.normal(0, [0.1, 0.1, 0.01]))).astype(np.float32) for _ in range(7)]
    got = _check(ctx, chain, [src], [tgt], gs, "many to one", jobs=[(0, 0)] * 8)
    assert (got[1] == 0).all()
