"""GPU parity of the two instances of the strip-sweep loop kernel's lane-per-query pass.  walk_pass exists twice in the
builds with clearance records: one instance for the iterations whose searches use the records' margin, carry the runner-up
distance and leave records (rec_on), one for the iterations before that, which does none of it; a workgroup-uniform branch
picks one per call.  The builds without records hold the second instance only.  Nothing a search decides changes, so pose,
status and iteration count of every job are compared with the brute-force kernel bit for bit, and the well-posed jobs with
the oracle's fp64-sum chain (status, iteration count, pose within 1e-6).

One list of jobs runs under both minimisers with 11 and 12 iterations (the two sides of SW_REC_MIN_ITER: the builds
without and with records), with 30 (records, triage pass, predicted quantile) and on the shipped chain, no differential
checker in the fixed chains, on every build of the loop kernel that takes the job's shape:
  * calls "tiers", "few", "one-size" and "brute" as in tests/test_gpu_icp_guess_frame.py.  At most one 1024-thread job per
    CU takes the 128-VGPR builds, which have no records: in these three calls only the one-wave and the four-wave build
    keep records;
  * call "crowd": sw_tiers = 0 and CUs + 8 small fillers behind the jobs, so that more 1024-thread jobs than CUs are
    in the call -> the 64-VGPR builds, two workgroups per CU, with records where the target is LDS-resident: the build
    the benchmark runs.
Targets of 8193 points take the build that reads the sorted target from HBM (no records).  The routes are asserted.

The jobs:
  * 63, 64, 65, 1023, 1024, 1025 and 4097 source points on targets of 300, 5000 and 8193 points;
  * the identity as the guess on a pair that is aligned already (a small and a 1024-thread shape): the step is small from
    the first iteration on, the records switch on at the second and nearly every walk is of the instance with records;
  * a turn of 0.35 rad with a shift of metres: many iterations without records, then the switch;
  * two pairs of parallel walls 4 cm apart, at right angles, the source between and around them: nearly every query has its
    runner-up on the other wall at almost the distance of its neighbour, so the clearance a record states is decided by
    the runner-up (what a search that drops it gets wrong).  Compared with the brute-force kernel only: between
    near-equidistant targets the order of the fp32 and the fp64 chain's choices need not agree.
Further cases: the same jobs with sw_rec = 0 (no records at all) give the default's bits; a chain with MedianDist (the
outlier-module build); a job shared by several workgroups, forced small through the sw_multi_* tuning (status and
iterations equal, pose within 1e-6 as before: the shares add their sums in share order); and, with the profile build, the
turned job as workgroup 0: its per-iteration words show iterations that settled no query by a record and later ones that
settled some, so both instances ran.

What the file can see: against a library built aside whose instance with records does not maintain the runner-up distance
(`second` stays infinite: the clearances it writes are too large) 8 of the 13 cases fail: the 12- and the 30-iteration
chains of both minimisers (call "crowd": 10 to 18 of the 27 jobs differ from the brute-force kernel, plain size jobs
among them), both sw_rec cases, the outlier-module build and the profiled run.  The 11-iteration and shipped chains and
the split job pass with it, as they must: their builds keep no records."""
import ctypes
import functools
import os
from multiprocessing.pool import ThreadPool

import numpy as np
import pytest

import oracle
from sonar_slam_amd import _lib as L
from sonar_slam_amd import icp_config, synth

import test_gpu_icp_guess_frame as gf
import test_gpu_icp_outliers as outl
import test_gpu_icp_sums_reduce as sums

pytestmark = pytest.mark.gpu

TOL_TIGHT = 1e-6
ONE_SIZE = dict(sw_tiers=0, sw_multi=0, sw_tiny=0)
SIZES = [(ns, nt) for nt in (300, 5000, 8193) for ns in (63, 64, 65, 1023, 1024, 1025, 4097)]
CHAINS = {"11": dict(max_iter=11, use_diff_checker=0), "12": dict(max_iter=12, use_diff_checker=0),
          "30": dict(max_iter=30, use_diff_checker=0), "shipped": {}}


def _walls(rng, n_src, n_tgt):
    """two double walls at right angles, 4 cm between the two faces of each; the source along both, moved a little"""
    def wall(n, gap):
        u = rng.uniform(2.0, 22.0, n)
        return np.c_[u, np.where(rng.random(n) < 0.5, 0.0, gap)]
    a = wall(n_tgt // 2, 0.04)
    b = wall(n_tgt - n_tgt // 2, 0.04)[:, ::-1] + [2.0, 0.0]
    tgt = np.r_[a, b] + rng.normal(0, 0.002, (n_tgt, 2))
    sa = np.c_[rng.uniform(2.0, 22.0, n_src // 2), rng.uniform(-0.03, 0.07, n_src // 2)]
    sb = np.c_[rng.uniform(-0.03, 0.07, n_src - n_src // 2) + 2.0, rng.uniform(2.0, 22.0, n_src - n_src // 2)]
    T = synth.pose_matrix(0.25, -0.15, 0.02)
    Ti = np.linalg.inv(T)
    src = np.r_[sa, sb] @ Ti[:2, :2].T + Ti[:2, 2]
    g = synth.pose_matrix(0.25 + 0.1, -0.15 - 0.08, 0.02 + 0.015)
    return src.astype(np.float32), tgt.astype(np.float32), g.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _jobs():
    """-> (sources, targets, jobs [(source, target)], guesses, names, oracle picks, one-wave filler, 1024-thread filler):
    built once, never changed"""
    rng = np.random.default_rng(2026)
    srcs, tgts, jobs, gs, names, picks = [], [], [], [], [], []

    def add(name, src, tgt, guess, ask_oracle):
        srcs.append(np.ascontiguousarray(src, np.float32))
        tgts.append(np.ascontiguousarray(tgt, np.float32))
        if ask_oracle:
            picks.append(len(jobs))
        jobs.append((len(srcs) - 1, len(srcs) - 1))
        gs.append(np.ascontiguousarray(guess, np.float32))
        names.append(name)

    for k, (ns, nt) in enumerate(SIZES):
        s, t, g, _ = synth.scan_pair(seed=9000 + k, n_src=ns, n_tgt=nt)
        add("size %d x %d" % (ns, nt), s, t, g, True)
    for k, (ns, nt) in enumerate([(300, 300), (1100, 5000)]):
        s, t, _, _ = synth.scan_pair(seed=9100 + k, n_src=ns, n_tgt=nt, motion=(0.0, 0.0, 0.0))
        add("aligned, identity guess %d" % ns, s, t, np.eye(3), True)
        s, t, g, _ = synth.scan_pair(seed=9110 + k, n_src=ns, n_tgt=nt, motion=(3.0, -2.0, 0.35))
        add("turned guess %d" % ns, s, t, g, True)
    for ns, nt in ((600, 1200), (2500, 5000)):
        s, t, g = _walls(rng, ns, nt)
        add("walls %d" % ns, s, t, g, False)
    fills = []
    for seed, n in ((9400, 24), (9401, 300)):
        fs, ft, fg, _ = synth.scan_pair(seed=seed, n_src=n, n_tgt=n)
        srcs.append(fs)
        tgts.append(ft)
        fills.append((len(srcs) - 1, fg))
    return srcs, tgts, jobs, gs, names, picks, fills[0], fills[1]


def _crowd(ctx, p, srcs, tgts, jobs, gs, fill, run=sums._run, **knobs):
    """the jobs and CUs + 8 fillers, every one on a 1024-thread build: more of them than CUs"""
    n_fill = ctx.n_cu + 8
    kn = dict(ONE_SIZE)
    kn.update(knobs)
    return run(ctx, p, srcs, tgts, jobs + [(fill[0], fill[0])] * n_fill, gs + [fill[1]] * n_fill, **kn)


def _calls(ctx, p, what, **knobs):
    """the four calls of the sweep kernel on the list of jobs, routes asserted -> {call: (T, status, iters, routes)}"""
    srcs, tgts, jobs, gs, names, _, (f0_pair, f0_guess), f2 = _jobs()
    n = len(jobs)
    shapes = [(len(srcs[a]), len(tgts[b])) for a, b in jobs]
    out = {}
    n_fill = 2 * ctx.n_cu + 16
    kn = dict(sw_tiny=0)
    kn.update(knobs)
    tiers = out["tiers"] = sums._run(ctx, p, srcs, tgts, jobs + [(f0_pair, f0_pair)] * n_fill, gs + [f0_guess] * n_fill, **kn)
    for (s, t), r, name in zip(shapes, tiers[3], names):
        if s <= gf.T0_SRC and t <= gf.T0_TGT:
            assert r == L.ICP_ROUTE_T0, (what, name, r)
        elif s <= gf.T1_SRC and t <= gf.T1_TGT:
            assert r == L.ICP_ROUTE_T1, (what, name, r)
        else:
            assert gf._big_ok(r, t), (what, name, r)
    assert (tiers[3][n:] == L.ICP_ROUTE_T0).all()
    few = out["few"] = sums._run(ctx, p, srcs, tgts, jobs, gs, **kn)
    for (s, t), r, name in zip(shapes, few[3], names):
        assert (r == L.ICP_ROUTE_T1) if s <= gf.T1_FEW_SRC and t <= gf.T1_TGT else gf._big_ok(r, t), (what, name, r)
    one = out["one-size"] = sums._run(ctx, p, srcs, tgts, jobs, gs, **dict(ONE_SIZE, **knobs))
    assert all(gf._big_ok(r, t) for (_, t), r in zip(shapes, one[3])), (what, np.unique(one[3]))
    crowd = out["crowd"] = _crowd(ctx, p, srcs, tgts, jobs, gs, f2, **knobs)
    assert all(gf._big_ok(r, t) for (_, t), r in zip(shapes, crowd[3])), (what, np.unique(crowd[3][:n]))
    assert (crowd[3][n:] == L.ICP_ROUTE_Q).all(), (what, np.unique(crowd[3][n:]))
    return out


@pytest.mark.parametrize("chain", list(CHAINS))
@pytest.mark.parametrize("minimizer", [0, 1])
def test_every_build_equals_the_brute_force_kernel(ctx, minimizer, chain):
    p = icp_config.shipped_params(minimizer=minimizer, **CHAINS[chain])
    srcs, tgts, jobs, gs, names, picks, _, _ = _jobs()
    n = len(jobs)
    what = "minimizer %d, chain %s" % (minimizer, chain)

    brute = sums._run(ctx, p, srcs, tgts, jobs, gs, variant=4)
    assert (brute[3] == L.ICP_ROUTE_BRUTE).all()
    got = _calls(ctx, p, what)
    for call in ("crowd", "tiers", "few", "one-size"):
        sums._same(got[call], brute, n, names, (what, call))

    # the cases are what they are built for
    st = dict(zip(names, brute[1]))
    assert all(st[nm] == 0 for nm in names), (what, {nm: int(st[nm]) for nm in names if st[nm] != 0})

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
            d = sums._pose_diff(got["crowd"][0][j], To)
            assert d < TOL_TIGHT, info + (d,)


@pytest.mark.parametrize("minimizer", [0, 1])
def test_without_records_the_same_bits(ctx, minimizer):
    """sw_rec = 0: the builds with records run with rec_on false throughout -- every walk is of the instance without
    records, in a build that holds both"""
    p = icp_config.shipped_params(minimizer=minimizer, **CHAINS["30"])
    _, _, jobs, _, names, _, _, _ = _jobs()
    what = "minimizer %d, sw_rec" % minimizer
    on = _calls(ctx, p, what)
    off = _calls(ctx, p, what + " = 0", sw_rec=0)
    for call in ("crowd", "tiers", "few", "one-size"):
        sums._same(off[call], on[call], len(jobs), names, (what, call))


def _subset(keep):
    srcs, tgts, jobs, gs, names, _, _, f2 = _jobs()
    sub = [j for j, nm in enumerate(names) if keep(nm)]
    return srcs, tgts, [jobs[j] for j in sub], [gs[j] for j in sub], [names[j] for j in sub], f2


def test_outlier_module_build(ctx):
    """a chain with MedianDist, 30 iterations: the 64-VGPR build with the outlier modules and records, and the four-wave one,
    against the brute-force kernel bit for bit and against the restatement of the chain"""
    p = icp_config.shipped_params(max_iter=30, use_diff_checker=0)
    ox = outl._ox(use_median=1, median_factor=3.0)
    srcs, tgts, jobs, gs, names, f2 = _subset(lambda nm: nm.startswith(("size 65 ", "size 1025 ", "size 4097 ", "aligned",
                                                                        "turned", "walls")))
    n = len(jobs)
    brute = outl._jobs(ctx, p, ox, srcs, tgts, jobs, gs, variant=4)
    assert (brute[3] == L.ICP_ROUTE_BRUTE).all()
    crowd = _crowd(ctx, p, srcs, tgts, jobs, gs, f2, run=lambda c, pp, *a, **kn: outl._jobs(c, pp, ox, *a, **kn))
    assert all(gf._big_ok(r, len(tgts[b])) for (_, b), r in zip(jobs, crowd[3])), crowd[3][:n]
    assert (crowd[3][n:] == L.ICP_ROUTE_Q).all()
    outl._same([x[:n] for x in crowd[:3]], brute[:3], "crowd")
    few = outl._jobs(ctx, p, ox, srcs, tgts, jobs, gs, sw_tiny=0)
    assert L.ICP_ROUTE_T1 in set(int(r) for r in few[3]), few[3]
    outl._same(few[:3], brute[:3], "few")
    picks = [j for j, nm in enumerate(names) if nm in ("size 65 x 300", "size 1025 x 5000", "turned guess 300",
                                                        "turned guess 1100")]
    assert len(picks) == 4
    outl._check_ref(p, ox, picks, srcs, tgts, jobs, gs, crowd, "median3")


def test_split_job(ctx):
    """jobs shared by several workgroups, forced at 1025 and 4097 source points, 12 iterations: split jobs keep no records,
    their builds hold the instance without them only"""
    p = icp_config.shipped_params(minimizer=1, max_iter=12, use_diff_checker=0)
    srcs, tgts, jobs, gs, names, _ = _subset(lambda nm: nm in ("size 1025 x 8193", "size 4097 x 8193"))
    brute = sums._run(ctx, p, srcs, tgts, jobs, gs, variant=4)
    with ctx.tuning(sw_multi_min_src=1024, sw_multi_share_min=64):
        got = sums._run(ctx, p, srcs, tgts, jobs, gs, sw_multi=1, sw_tiers=1)
    assert (got[3] == L.ICP_ROUTE_SPLIT).all(), got[3]
    assert (brute[1] == 0).all(), brute[1]
    assert np.array_equal(got[1], brute[1]) and np.array_equal(got[2], brute[2]), (got[1], brute[1], got[2], brute[2])
    for j, nm in enumerate(names):
        d = sums._pose_diff(got[0][j], brute[0][j])
        assert d < TOL_TIGHT, (nm, d)


def test_both_instances_ran(ctx):
    """the profile build (64 VGPRs, records) with the turned job as workgroup 0: word 17 + 2 i of the profile holds, in
    bits 16..31, how many queries of iteration i a clearance record settled.  Iterations without any (but the first, which
    has no previous neighbour to hold a record against) and later iterations with some: the searches of the first ran
    without records or before any existed, those of the second with them.  The profiled run equals the brute-force kernel."""
    p = icp_config.shipped_params(minimizer=1, **CHAINS["30"])
    srcs, tgts, jobs, gs, names, f2 = _subset(lambda nm: nm in ("turned guess 1100", "aligned, identity guess 1100"))
    assert names[0] == "aligned, identity guess 1100" and names[1] == "turned guess 1100"
    jobs, gs, names = jobs[::-1], gs[::-1], names[::-1]
    brute = sums._run(ctx, p, srcs, tgts, jobs, gs, variant=4)
    cyc = (ctypes.c_longlong * 96)()
    ctx._check(ctx.lib.sfe_icp_get_profile(ctx.handle, 1, None))
    try:
        got = _crowd(ctx, p, srcs, tgts, jobs, gs, f2)
        ctx.sync()
    finally:
        ctx._check(ctx.lib.sfe_icp_get_profile(ctx.handle, 0, cyc))
    assert (got[3] == L.ICP_ROUTE_Q).all(), np.unique(got[3])
    sums._same(got, brute, 2, names, "profiled crowd")
    it = int(got[2][0])
    assert it == 30, it
    hits = [int((cyc[17 + 2 * i] >> 16) & 0xFFFF) for i in range(it)]
    print("settled by a clearance record, per iteration of the turned job:", hits)
    first = next((i for i, h in enumerate(hits) if h > 0), None)
    assert first is not None and first >= 4, hits          # several iterations of walks without records ...
    assert sum(1 for h in hits[first:] if h > 0) >= 5, hits  # ... then with them
