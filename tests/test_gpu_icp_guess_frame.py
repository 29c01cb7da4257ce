"""GPU parity of the strip-sweep loop kernel's guess-frame positions.  The kernel forms r = T0 * src (T0 = mean^-1 * guess)
once per job, in the sort at its start, and keeps it twice: in the 16-byte slot record {r.x, r.y, query, clearance record}
that the fresh pass and the triage pass stream through, and in Q.rsrc under the query's own index for every later visit
(second pass, cooperative tier, both loops of the error-minimiser sums).  The iterations apply T_iter to the stored r; the
brute-force kernel still recomputes T_iter * (T0 * src) from the source point at every use.  So pose, status and
iteration count of every job are compared with the brute-force kernel bit for bit, and the well-posed jobs with the
oracle's fp64-sum chain (status, iteration count, pose within 1e-6).

One list of jobs runs under both minimisers with 1, 3 and 30 iterations (30 turns the clearance records, the triage pass
and the predicted quantile on) and on the shipped chain, on every build of the loop kernel that takes the job's shape
(the launcher's rule, as tests/test_gpu_icp_tiers.py selects it):
  * call "tiers": the jobs and 2 x CUs + 16 small fillers -> the one-wave build (at most 384 x 512 points), the four-wave
    build (at most 2048 x 2048), the 1024-thread builds for the rest;
  * call "few": the jobs alone -> the four-wave build for at most 320 source points, a 1024-thread build for the rest;
  * call "one-size": tuning sw_tiers = 0 -> every job on a 1024-thread build;
  * call "brute": the brute-force kernel.
Targets of 8193 points take the build that reads the sorted target from HBM.  The routes are asserted.

The jobs:
  * 1, 63, 64, 65, 1023, 1024, 1025, 2049 and 4097 source points: one slot record more or less than a slice of a 64-, 256-
    and 1024-thread workgroup, where the record requested a slice ahead is the last one, or is not requested;
  * targets of 3, 300, 5000 and 8193 points;
  * guesses: the identity; a turn of 0.35 rad with a shift of metres; a shift of 1e-7 with -0.0 entries; eight guesses on one
    source / target pair in one call (small and 1024-thread builds), each held to its own brute-force result -- Q.rsrc is
    per job, and jobs that share a source cloud must not share it; and 24 guesses on one small pair, because eight
    workgroups in a row run on eight dies, each with an L2 of its own in front of the scratch;
  * a source with one NaN x and one NaN y, in different points (arrays with equal_nan; NaN payloads are not part of the
    contract).
The oracle is asked about every job but those on the three-point target (rank-deficient: the order of the sums decides the
result) and the NaN jobs.

Further cases: a chain with MedianDist (the outlier-module build) against the brute-force kernel and the restatement of
the chain; and jobs shared by several workgroups, forced at a small size through the sw_multi_* tuning: every share forms
r for its own queries.  The shares add their sums in share order, not in that of a 1024-thread workgroup, so a split job
equals the brute-force kernel in status and iteration count and within 1e-6 in pose, as it did before.

What the file can see: against a library built aside whose Q.rsrc is indexed by the job's source offset instead of its
query offset, all eight cases of the first test fail on the 24-guess jobs, on every build.  The eight-guess jobs alone did
not notice (the first version of this file passed with that library): each of the eight workgroups read back its own
writes from its die's L2.  The 24-guess jobs were added for it."""
import functools
import os
from multiprocessing.pool import ThreadPool

import numpy as np
import pytest

import oracle
from sonar_slam_amd import _lib as L
from sonar_slam_amd import icp_config, synth

import test_gpu_icp_outliers as outl
import test_gpu_icp_sums_reduce as sums

pytestmark = pytest.mark.gpu

TOL_TIGHT = 1e-6
ONE_SIZE = dict(sw_tiers=0, sw_multi=0, sw_tiny=0)
T0_SRC, T0_TGT, T1_SRC, T1_TGT, T1_FEW_SRC = 384, 512, 2048, 2048, 320   # the launcher's limits (sfe_icp_sweep.hip)
TCAP = 8192                                                              # targets beyond it stay in HBM
BIG = (L.ICP_ROUTE_Q, L.ICP_ROUTE_LDS)
SIZES = [(1, 300), (63, 300), (64, 300), (65, 300), (1023, 300), (1024, 300), (1025, 300), (2049, 300), (4097, 300),
         (65, 5000), (1025, 5000), (4097, 5000), (64, 8193), (1025, 8193), (4097, 8193)]
THREE = [1, 65, 1025]                                                    # source sizes on the three-point target
TINY_GUESS = np.array([[1.0, -0.0, 1e-7], [0.0, 1.0, -0.0], [0.0, 0.0, 1.0]], np.float32)


@functools.lru_cache(maxsize=None)
def _jobs():
    """-> (sources, targets, jobs [(source, target)], guesses, names, oracle picks, filler): built once, never changed"""
    rng = np.random.default_rng(2025)
    srcs, tgts, jobs, gs, names, picks = [], [], [], [], [], []

    def add(name, src, tgt, guess, ask_oracle, pair=None):
        if pair is None:
            srcs.append(np.ascontiguousarray(src, np.float32))
            tgts.append(np.ascontiguousarray(tgt, np.float32))
            pair = len(srcs) - 1
        if ask_oracle:
            picks.append(len(jobs))
        jobs.append((pair, pair))
        gs.append(np.ascontiguousarray(guess, np.float32))
        names.append(name)
        return pair

    for k, (ns, nt) in enumerate(SIZES):
        s, t, g, _ = synth.scan_pair(seed=8000 + k, n_src=ns, n_tgt=nt)
        add("size %d x %d" % (ns, nt), s, t, g, True)
    for ns in THREE:
        t = rng.uniform(-8, 8, (3, 2)).astype(np.float32)
        s = t[rng.integers(0, 3, ns)] + rng.normal(0, 0.1, (ns, 2)) + rng.uniform(-0.3, 0.3, 2)
        add("three-point target %d" % ns, s, t, synth.pose_matrix(*rng.normal(0, [0.3, 0.3, 0.05])), False)
    # the guesses, each on a small and on a 1024-thread shape
    for k, (ns, nt) in enumerate([(300, 300), (1100, 5000)]):
        s, t, _, _ = synth.scan_pair(seed=8100 + k, n_src=ns, n_tgt=nt, motion=(0.05, -0.03, 0.01))
        add("identity guess %d" % ns, s, t, np.eye(3), True)
        s, t, g, _ = synth.scan_pair(seed=8110 + k, n_src=ns, n_tgt=nt, motion=(3.0, -2.0, 0.3))
        add("turned guess %d" % ns, s, t, g, True)
        s, t, _, _ = synth.scan_pair(seed=8120 + k, n_src=ns, n_tgt=nt, motion=(0.0, 0.0, 0.0))
        add("1e-7 guess %d" % ns, s, t, TINY_GUESS, True)
    # eight guesses on one pair
    for k, (ns, nt) in enumerate([(300, 300), (1100, 1500)]):
        s, t, g, _ = synth.scan_pair(seed=8200 + k, n_src=ns, n_tgt=nt)
        pair = None
        for i in range(8):
            gi = g.astype(np.float64) @ synth.pose_matrix(*rng.normal(0, [0.1, 0.1, 0.01]))
            pair = add("guess %d of eight, %d" % (i, ns), s, t, gi, True, pair)
    # ... and 24 guesses on one pair: the workgroups of a launch are dealt to the device's eight dies in turn and every die
    # keeps its own L2 in front of the scratch, so eight jobs that wrongly shared an array would each see their own
    # writes; of 24 consecutive jobs three run on every die
    s, t, g, _ = synth.scan_pair(seed=8210, n_src=300, n_tgt=300)
    pair = None
    for i in range(24):
        gi = g.astype(np.float64) @ synth.pose_matrix(*rng.normal(0, [0.1, 0.1, 0.01]))
        pair = add("guess %d of 24" % i, s, t, gi, True, pair)
    # a NaN x and a NaN y, in different points
    for ns, nt, ax, ay in ((300, 300, 77, 140), (1025, 5000, 1024, 3)):
        s, t, g, _ = synth.scan_pair(seed=8300 + ns, n_src=ns, n_tgt=nt)
        s[ax, 0] = np.nan
        s[ay, 1] = np.nan
        add("NaN %d" % ns, s, t, g, False)
    # fillers (at the end, results unused): small jobs that keep the one-wave build live in the call "tiers"
    fs, ft, fg, _ = synth.scan_pair(seed=8400, n_src=24, n_tgt=24)
    srcs.append(fs)
    tgts.append(ft)
    return srcs, tgts, jobs, gs, names, picks, (len(srcs) - 1, fg)


def _big_ok(r, nt):
    return r == L.ICP_ROUTE_GLB if nt > TCAP else r in BIG


CHAINS = {"1": dict(max_iter=1, use_diff_checker=0), "3": dict(max_iter=3, use_diff_checker=0),
          "30": dict(max_iter=30, use_diff_checker=0), "shipped": {}}


@pytest.mark.parametrize("chain", list(CHAINS))
@pytest.mark.parametrize("minimizer", [0, 1])
def test_every_build_equals_the_brute_force_kernel(ctx, minimizer, chain):
    p = icp_config.shipped_params(minimizer=minimizer, **CHAINS[chain])
    srcs, tgts, jobs, gs, names, picks, (fill_pair, fill_guess) = _jobs()
    n = len(jobs)
    shapes = [(len(srcs[a]), len(tgts[b])) for a, b in jobs]
    what = "minimizer %d, chain %s" % (minimizer, chain)

    brute = sums._run(ctx, p, srcs, tgts, jobs, gs, variant=4)
    assert (brute[3] == L.ICP_ROUTE_BRUTE).all()

    n_fill = 2 * ctx.n_cu + 16
    tiers = sums._run(ctx, p, srcs, tgts, jobs + [(fill_pair, fill_pair)] * n_fill, gs + [fill_guess] * n_fill, sw_tiny=0)
    for (s, t), r, name in zip(shapes, tiers[3], names):
        if s <= T0_SRC and t <= T0_TGT:
            assert r == L.ICP_ROUTE_T0, (what, name, r)
        elif s <= T1_SRC and t <= T1_TGT:
            assert r == L.ICP_ROUTE_T1, (what, name, r)
        else:
            assert _big_ok(r, t), (what, name, r)
    assert (tiers[3][n:] == L.ICP_ROUTE_T0).all()
    sums._same(tiers, brute, n, names, (what, "tiers"))

    few = sums._run(ctx, p, srcs, tgts, jobs, gs, sw_tiny=0)
    for (s, t), r, name in zip(shapes, few[3], names):
        assert (r == L.ICP_ROUTE_T1) if s <= T1_FEW_SRC and t <= T1_TGT else _big_ok(r, t), (what, name, r)
    sums._same(few, brute, n, names, (what, "few"))

    one = sums._run(ctx, p, srcs, tgts, jobs, gs, **ONE_SIZE)
    assert all(_big_ok(r, t) for (_, t), r in zip(shapes, one[3])), (what, np.unique(one[3]))
    sums._same(one, brute, n, names, (what, "one-size"))

    # the cases are what they are built for
    st = dict(zip(names, brute[1]))
    ok = [nm for nm in names if nm.startswith(("size", "identity", "turned", "1e-7", "guess")) and not nm.startswith("size 1 ")]
    assert all(st[nm] == 0 for nm in ok), (what, {nm: int(st[nm]) for nm in ok if st[nm] != 0})

    op = oracle.shipped_icp_params(precision=1, **p.as_dict())

    def ask(j):
        a, b = jobs[j]
        return oracle.icp(srcs[a], tgts[b], gs[j], op)

    with sums._kdtree(), ThreadPool(max(1, min(16, os.cpu_count() or 1))) as tp:
        ref = tp.map(ask, picks)
    for j, (sto, To, ito) in zip(picks, ref):
        info = (what, names[j])
        assert brute[1][j] == sto and brute[2][j] == ito, info + (int(brute[1][j]), sto, int(brute[2][j]), ito)
        if sto == 0:
            d = sums._pose_diff(tiers[0][j], To)
            assert d < TOL_TIGHT, info + (d,)


def _subset(keep):
    """the jobs whose name passes `keep`, as (sources, targets, jobs, guesses, names)"""
    srcs, tgts, jobs, gs, names, _, _ = _jobs()
    sub = [j for j, nm in enumerate(names) if keep(nm)]
    return srcs[:-1], tgts[:-1], [jobs[j] for j in sub], [gs[j] for j in sub], [names[j] for j in sub]


def test_outlier_module_build(ctx):
    """a chain with MedianDist: the build with the outlier modules, 30 iterations, against the brute-force kernel bit for
    bit and against the restatement of the chain"""
    p = icp_config.shipped_params(max_iter=30, use_diff_checker=0)
    ox = outl._ox(use_median=1, median_factor=3.0)
    srcs, tgts, jobs, gs, names = _subset(lambda nm: nm.startswith(("size 65 ", "size 1025 ", "size 4097 ", "guess", "NaN")))
    brute = outl._jobs(ctx, p, ox, srcs, tgts, jobs, gs, variant=4)
    assert (brute[3] == L.ICP_ROUTE_BRUTE).all()
    one = outl._jobs(ctx, p, ox, srcs, tgts, jobs, gs, **ONE_SIZE)
    assert all(_big_ok(r, len(tgts[b])) for (_, b), r in zip(jobs, one[3])), one[3]
    outl._same(one[:3], brute[:3], "one-size")
    few = outl._jobs(ctx, p, ox, srcs, tgts, jobs, gs, sw_tiny=0)
    assert L.ICP_ROUTE_T1 in set(int(r) for r in few[3]), few[3]
    outl._same(few[:3], brute[:3], "few")
    picks = [j for j, nm in enumerate(names) if nm in ("size 65 x 300", "size 1025 x 300", "guess 3 of eight, 300",
                                                        "guess 5 of eight, 1100")]
    assert len(picks) == 4
    outl._check_ref(p, ox, picks, srcs, tgts, jobs, gs, one, "median3")


@pytest.mark.parametrize("minimizer", [0, 1])
def test_split_jobs(ctx, minimizer):
    """jobs shared by several workgroups, forced at 1025 and 4097 source points: two guesses on each source cloud"""
    p = icp_config.shipped_params(minimizer=minimizer, max_iter=8, use_diff_checker=0)
    srcs, tgts, jobs, gs, names = _subset(lambda nm: nm in ("size 1025 x 8193", "size 4097 x 8193"))
    rng = np.random.default_rng(5)
    jobs = jobs + jobs
    gs = gs + [(g.astype(np.float64) @ synth.pose_matrix(*rng.normal(0, [0.1, 0.1, 0.01]))).astype(np.float32) for g in gs]
    names = names + [nm + ", second guess" for nm in names]
    brute = sums._run(ctx, p, srcs, tgts, jobs, gs, variant=4)
    with ctx.tuning(sw_multi_min_src=1024, sw_multi_share_min=64):
        got = sums._run(ctx, p, srcs, tgts, jobs, gs, sw_multi=1, sw_tiers=1)
    assert (got[3] == L.ICP_ROUTE_SPLIT).all(), got[3]
    assert (brute[1] == 0).all(), brute[1]
    assert np.array_equal(got[1], brute[1]) and np.array_equal(got[2], brute[2]), (got[1], brute[1], got[2], brute[2])
    for j, nm in enumerate(names):
        d = sums._pose_diff(got[0][j], brute[0][j])
        assert d < TOL_TIGHT, (nm, d)
