"""GPU: every value of the strip-sweep ICP knobs (sfe_tune sw_*) computes the results of the default setting.

include/sonarfe.h promises that every setting of the launcher knobs computes the same results, and the knob tools
(tools/icp_knobs.py, icp_env_sweep.py, stage_times.py --tune) compare settings on that promise.  At the defaults the
exactness-critical fallbacks of the loop kernel stay cold: the cooperative tier (queries that exhaust the second-pass
budget), repeated search rounds after the first iteration (a cap margin that turns out too small), strip tables of
64 strips with empty and one-point strips, the union scan after the first iteration.  The edges of every knob's range
drive them.  Here each knob on its own at its edges (GRID) and two combined settings (STARVED, GENEROUS) run

  (a) the every-job-class call of test_gpu_icp_tiers (tiny, one-wave, four-wave, Q, LDS and GLB jobs),
  (b) a tie-heavy call: targets on a coarse grid, mirrored about the origin (their mean is exactly 0, so centring moves
      no coordinate), with duplicated points and whole lines of equal x and equal y; sources on the half-way points
      between targets and identity guesses, so the first iteration meets exact ties everywhere and the lowest-index
      rule decides,
  (c) one 20 000 x 12 000 pair split over several workgroups,

under the shipped chain, the two 30-iteration chains (the clearance-record builds) and a MedianDist + MinDist chain (the
OX build).  (a) and (b) must equal the default-knob run bit for bit (T, status, iterations, routes); the default run
is checked once per chain and batch against the fp64-sum oracle or the numpy restatement (tests/icp_chain_ref.py), and
the two combined settings against the brute-force kernel bit for bit.  (c) keeps the split route's contract against
the unsplit default run.  A profiled run shows that the extremes reach the paths they aim at, and that the PROF builds
compute what the shipped builds compute; a run with icp_debug = 1 shows that no loop watchdog cut a search short."""
import ctypes

import numpy as np
import pytest

from sonar_slam_amd import _lib as L
from sonar_slam_amd import icp_config, pcl, synth

import test_gpu_icp_outliers as outl
import test_gpu_icp_tiers as tiers

pytestmark = pytest.mark.gpu

TOL_TIGHT = 1e-6
P20 = 1 << 20
# the defaults of sfe_tuning (sfe_internal.h; LAB_NOTEBOOK Appendix A)
DEFAULTS = dict(sw_budget=128, sw_budget_a=6, sw_rtrips=4, sw_margin=15, sw_strip_pts=96, sw_union_iters=1,
                sw_union_max=768, sw_recm=8, sw_reck=3.0, sw_cache=1, sw_rec=1, sw_multi=1, sw_multi_g=0,
                sw_multi_share_min=1024, sw_multi_min_src=8192, sw_tiers=1, sw_tiny=1, icp_debug=0)
GRID = [dict(sw_budget=1), dict(sw_budget=2), dict(sw_budget=65535), dict(sw_budget_a=1), dict(sw_budget_a=65535),
        dict(sw_rtrips=1), dict(sw_rtrips=255), dict(sw_margin=0), dict(sw_margin=255),
        dict(sw_strip_pts=1), dict(sw_strip_pts=7), dict(sw_strip_pts=P20),
        dict(sw_union_iters=0), dict(sw_union_iters=255), dict(sw_union_max=0), dict(sw_union_max=65535),
        dict(sw_recm=1), dict(sw_recm=100), dict(sw_reck=0), dict(sw_reck=0.5), dict(sw_reck=1000),
        dict(sw_cache=0, sw_rec=1), dict(sw_cache=0, sw_rec=0), dict(sw_rec=0)]
STARVED = dict(sw_budget=1, sw_budget_a=1, sw_rtrips=1, sw_margin=0, sw_strip_pts=1, sw_recm=1, sw_reck=0)
GENEROUS = dict(sw_budget=65535, sw_budget_a=65535, sw_rtrips=255, sw_margin=255, sw_strip_pts=P20, sw_union_iters=255,
                sw_union_max=65535, sw_recm=100, sw_reck=1000)

CHAINS = {  # name -> (sfe_icp_params over the shipped chain, sfe_icp_outliers or None)
    "shipped": ({}, None),
    "p2p30": (tiers.P2P_REC, None),
    "p2plane30": (tiers.P2PLANE_REC, None),
    "median2_mindist": (dict(use_trimmed_filter=0), dict(use_median=1, median_factor=2.0, use_min_dist=1, min_dist=0.02)),
}


def _chain(name):
    over, oxkw = CHAINS[name]
    return icp_config.shipped_params(**over), (outl._ox(**oxkw) if oxkw else None)


def _call(ctx, chain, batch, variant=0, **knobs):
    """one compute_jobs call of `batch` = (srcs, tgts, jobs, guesses) -> (T, status, iters, routes)"""
    p, ox = _chain(chain)
    st, T, it, routes = outl._jobs(ctx, p, ox, *batch, variant, **knobs)
    return T, st, it, routes


def _same(a, b, what):
    """bit for bit: T, status, iterations and the route of every job"""
    tiers._same(a, b, what)
    assert np.array_equal(a[3], b[3]), (what, "routes", np.flatnonzero(a[3] != b[3])[:10])


def _check_reference(chain, picks, batch, got, what):
    """the picked jobs against the plain high-precision reference of the chain: status and iterations equal, pose
    within 1e-6 (the fp64-sum oracle; chains with outlier modules: the numpy restatement)"""
    p, ox = _chain(chain)
    if ox is None:
        tiers._check_oracle(p, picks, *batch, got, what)
    else:
        outl._check_ref(p, ox, picks, *batch, (got[1], got[0], got[2], got[3]), what)


def _assert_defaults(ctx):
    """the session context is shared: every knob back at its default"""
    for name, value in DEFAULTS.items():
        assert ctx.tune(name, value) == value, name


def _subset(batch, sub):
    srcs, tgts, jobs, gs = batch
    return srcs, tgts, [jobs[j] for j in sub], [gs[j] for j in sub]


def _knob_id(knobs):
    return "starved" if knobs is STARVED else "generous" if knobs is GENEROUS else \
        ",".join("%s=%g" % kv for kv in knobs.items())


# ---- the batches -------------------------------------------------------------------------------------------------

def _tie_pair(rng, n_tgt, n_src):
    """a target on the 0.5 m grid, mirrored about the origin (mean exactly 0), with duplicated points, and a source on
    its points and the half-way points between them (offsets of 0.25 m along x, y or both: two or four targets at
    exactly the same distance)"""
    h = n_tgt // 2
    half = rng.integers(-10, 11, (h, 2)).astype(np.float32) * np.float32(0.5)
    dup = rng.random(h) < 0.2
    half[dup] = half[rng.integers(0, h, int(dup.sum()))]
    tgt = np.concatenate([half, -half] + ([np.zeros((1, 2), np.float32)] if n_tgt % 2 else []))
    off = np.array([(0.25, 0), (-0.25, 0), (0, 0.25), (0, -0.25), (0.25, 0.25), (-0.25, 0.25), (0.25, -0.25),
                    (-0.25, -0.25), (0, 0)], np.float32)
    src = tgt[rng.integers(0, len(tgt), n_src)] + off[rng.integers(0, len(off), n_src)]
    assert np.sum(tgt.astype(np.float64), axis=0).tolist() == [0.0, 0.0]
    return np.ascontiguousarray(src, np.float32), np.ascontiguousarray(tgt, np.float32)


def _tie_batch(ctx):
    """2 x CUs jobs of one-wave shape (tiny on the short chains) and 32 more: four-wave jobs on small (150..500 points)
    and larger targets and 1024-thread jobs on small targets; the first copy of every pair with the identity guess
    -> (srcs, tgts, jobs, guesses, n0 = the pairs of one-wave shape)"""
    rng = np.random.default_rng(51)
    sizes = [(int(rng.integers(340, 385)), int(rng.integers(360, 513))) for _ in range(8)]            # one wave
    n0 = len(sizes)
    sizes += [(int(rng.integers(600, 2049)), int(rng.integers(150, 501))) for _ in range(10)]         # four waves
    sizes += [(int(rng.integers(600, 2049)), int(rng.integers(1000, 2049))) for _ in range(4)]
    sizes += [(int(rng.integers(2500, 3001)), int(rng.integers(150, 501))) for _ in range(2)]         # 1024 threads
    srcs, tgts = [], []
    for s, t in sizes:
        a, b = _tie_pair(rng, t, s)
        srcs.append(a)
        tgts.append(b)
    eye = np.eye(3, dtype=np.float32)

    def tile(lo, hi, n):
        d = hi - lo
        jobs = [(lo + j % d, lo + j % d) for j in range(n)]
        gs = [eye if j < d else synth.pose_matrix(*rng.normal(0, [0.05, 0.05, 0.01])).astype(np.float32) for j in range(n)]
        return jobs, gs

    jobs, gs = tile(0, n0, 2 * ctx.n_cu)
    j1, g1 = tile(n0, len(sizes), 32)
    return srcs, tgts, jobs + j1, gs + g1, n0


@pytest.fixture(scope="module")
def batches(ctx):
    srcs, tgts, jobs, gs, n, _ = tiers._every_class_batch(ctx)
    mixed = (srcs, tgts, jobs, gs)
    srcs, tgts, jobs, gs, n0 = _tie_batch(ctx)
    return {"mixed": (mixed, n), "ties": ((srcs, tgts, jobs, gs), n0)}


def _want_routes(ctx, chain, name, batch, n):
    """the launcher's rule for the batch: _small_routes for jobs of at most 2048 x 2048, the 1024-thread routes beyond"""
    p, _ = _chain(chain)
    srcs, tgts, jobs, _ = batch
    shapes = [(len(srcs[a]), len(tgts[b])) for a, b in jobs]
    want = tiers._small_routes(shapes, p, ctx.n_cu)
    if name == "mixed":
        return want[:n] + tiers.BIG_ROUTES
    return [L.ICP_ROUTE_Q if r is None else r for r in want]


def _picks(routes, batch):
    """the smallest job (source points) of every route, and the first two jobs of every route"""
    srcs = batch[0]
    jobs = batch[2]
    picks = set(outl._route_picks(routes))
    for r in set(int(x) for x in routes):
        idx = np.flatnonzero(routes == r)
        picks.add(int(min(idx, key=lambda j: len(srcs[jobs[j][0]]))))
    return sorted(picks)


# ---- 1, 2 (a) (b), 3, 4: the grid -------------------------------------------------------------------------------

@pytest.mark.parametrize("chain", sorted(CHAINS))
@pytest.mark.parametrize("name", ["mixed", "ties"])
def test_every_knob_value_returns_the_default_results(ctx, batches, name, chain):
    """every GRID value and the two combined settings: bit for bit the default-knob run of the same call, whose picks
    of every route match the high-precision reference; STARVED and GENEROUS also bit for bit the brute-force kernel
    on a subset of the jobs"""
    batch, n = batches[name]
    _assert_defaults(ctx)
    base = _call(ctx, chain, batch)
    routes = list(base[3])
    assert routes == _want_routes(ctx, chain, name, batch, n), (name, chain)
    if name == "mixed":
        assert {L.ICP_ROUTE_Q, L.ICP_ROUTE_LDS, L.ICP_ROUTE_GLB} <= set(routes)
    else:
        assert {L.ICP_ROUTE_T1, L.ICP_ROUTE_Q} <= set(routes)
        assert L.ICP_ROUTE_T0 in set(routes) or chain in ("shipped", "median2_mindist")
    picks = _picks(base[3], batch)
    _check_reference(chain, picks, batch, base, (name, chain))
    assert (base[1][picks] == 0).sum() >= len(picks) // 2           # mostly converged: the poses are compared
    for knobs in GRID + [STARVED, GENEROUS]:
        got = _call(ctx, chain, batch, **knobs)
        _same(got, base, (name, chain, _knob_id(knobs)))
    _assert_defaults(ctx)
    sub = sorted(set(range(0, len(batch[2]), 23)) | set(range(len(batch[2]) - 6, len(batch[2]))))
    for knobs in (STARVED, GENEROUS):
        brute = _call(ctx, chain, _subset(batch, sub), variant=4, **knobs)
        assert (brute[3] == L.ICP_ROUTE_BRUTE).all()
        tiers._same(brute, tuple(x[sub] for x in base[:3]), (name, chain, _knob_id(knobs), "brute force"))
    _assert_defaults(ctx)


# ---- 2 (c): the split job ---------------------------------------------------------------------------------------

SPLIT_SETTINGS = [STARVED, GENEROUS, dict(sw_multi_g=1), dict(sw_multi_g=16), dict(sw_multi_share_min=1),
                  dict(sw_multi_min_src=0)]


@pytest.fixture(scope="module")
def split_pair():
    """test_gpu_icp's split pair: 20 000 x 12 000 points, far outliers, three guesses"""
    src, tgt, guess, _ = synth.scan_pair(seed=41, n_src=20000, n_tgt=12000)
    src[::53] += 45.0
    base = synth.pose_of(guess)
    rng = np.random.default_rng(10)
    guesses = [synth.pose_matrix(base[0] + dx, base[1] + dy, base[2] + dt).astype(np.float32)
               for dx, dy, dt in rng.normal(0, [0.3, 0.3, 0.05], (3, 3))]
    return src, tgt, guesses


@pytest.mark.parametrize("over", [{}, tiers.P2PLANE_REC], ids=["shipped", "p2plane30"])
def test_split_job_under_every_setting(ctx, split_pair, over):
    """The split job under the sweep-knob extremes and the split knobs' edges: status and iterations of the unsplit
    default run, pose within 1e-6 (the shares add their sums in another order).  sw_multi_g = 1 leaves the job whole
    (the GLB route): bit for bit.  Unsplit under the extremes, the GLB route is bit for bit the default too."""
    src, tgt, guesses = split_pair
    p = icp_config.shipped_params(**over)
    icp = pcl.ICP(ctx)
    icp.setParams(p)
    _assert_defaults(ctx)
    with ctx.tuning(sw_multi=0):
        ref = icp.compute_batch(src, tgt, guesses)
    assert list(ctx.icp_routes(3)) == [L.ICP_ROUTE_GLB] * 3
    assert all(m == "success" for m in ref[0]), ref[0]
    for knobs in SPLIT_SETTINGS:
        what = (over, _knob_id(knobs))
        with ctx.tuning(**knobs):
            got = icp.compute_batch(src, tgt, guesses)
            routes = list(ctx.icp_routes(3))
            if knobs in (STARVED, GENEROUS):
                with ctx.tuning(sw_multi=0):
                    whole = icp.compute_batch(src, tgt, guesses)
                assert whole[0] == ref[0] and np.array_equal(whole[1], ref[1]) and np.array_equal(whole[2], ref[2]), what
        assert got[0] == ref[0] and np.array_equal(got[2], ref[2]), what + (got[0], got[2], ref[2])
        if knobs.get("sw_multi_g") == 1:
            assert routes == [L.ICP_ROUTE_GLB] * 3, what
            assert np.array_equal(got[1], ref[1]), what
        else:
            assert routes == [L.ICP_ROUTE_SPLIT] * 3, what
            assert max(tiers._pose_diff(x, y) for x, y in zip(got[1], ref[1])) < TOL_TIGHT, what
    _assert_defaults(ctx)


# ---- 5: the extremes reach their paths; the profiled builds ------------------------------------------------------

def _profiled(ctx, fn):
    """fn() with the loop kernel's profile on -> (fn's result, the 96 values of the last profiled launch)"""
    cyc = (ctypes.c_longlong * 96)()
    ctx._check(ctx.lib.sfe_icp_get_profile(ctx.handle, 1, None))
    try:
        out = fn()
        ctx.sync()
    finally:
        ctx._check(ctx.lib.sfe_icp_get_profile(ctx.handle, 0, cyc))
    return out, list(cyc)


def _uniform_batch(ctx, n_jobs, n_src, n_tgt, seed, outliers=0.2):
    pairs = [synth.scan_pair(seed=seed + i, n_src=n_src, n_tgt=n_tgt, outliers=outliers) for i in range(4)]
    jobs, gs = tiers._tile(pairs, n_jobs, np.random.default_rng(seed))
    return [q[0] for q in pairs], [q[1] for q in pairs], jobs, gs


def test_extremes_reach_their_paths_and_profiled_builds_agree(ctx):
    """More jobs than CUs with LDS-resident targets (the 1024-thread builds that are not `wide`, whose profiled
    instantiations exist), an 11-iteration fixed chain (no clearance records).  35 % of the source points are outliers,
    so the trimmed quantile (rank 0.8) falls among distances the error minimiser does not shrink: it moves up and down
    from one iteration to the next, and the next iteration's cap (the limit x (1 + margin), at least Cinit / 16) decides
    whether a second search round is needed.  (On clouds whose limit stays below Cinit / 16 the margin changes nothing.)
    Counters [9]..[12] are workgroup 0's, i.e. job 0's, which every knob below affects:
      sw_budget = 1   -> [10] (queries handed to the cooperative tier) and [81] (its candidate evaluations) non-zero,
      sw_budget_a = 1 -> [11] (queries handed to the second pass) above the default's,
      sw_margin = 0   -> [9] (search rounds) above the default's.
    Every profiled run is bit for bit the unprofiled default run; so are the profiled builds of the other routes that
    have one: Q with clearance records, LDS, and the four-wave build without records."""
    p = icp_config.shipped_params(max_iter=11, use_diff_checker=0)
    batch = _uniform_batch(ctx, ctx.n_cu + 8, 2400, 2400, 5100, outliers=0.35)
    _assert_defaults(ctx)
    run = lambda **kn: outl._jobs(ctx, p, None, *batch, **kn)      # noqa: E731 -> (status, T, iters, routes)
    base = run()
    assert (base[3] == L.ICP_ROUTE_Q).all(), np.unique(base[3])
    cnt = {}
    for key, knobs in (("default", {}), ("budget", dict(sw_budget=1)), ("budget_a", dict(sw_budget_a=1)),
                       ("margin", dict(sw_margin=0))):
        got, cnt[key] = _profiled(ctx, lambda: run(**knobs))
        outl._same(got, base, ("profiled", key))
        assert cnt[key][84] == int(base[2].sum()), key              # [84] iterations of the whole launch
    assert cnt["budget"][10] > 0 and cnt["budget"][81] > 0, (cnt["default"][10], cnt["budget"][10], cnt["budget"][81])
    assert cnt["budget_a"][11] > cnt["default"][11], (cnt["default"][11], cnt["budget_a"][11])
    assert cnt["margin"][9] > cnt["default"][9], (cnt["default"][9], cnt["margin"][9])
    _assert_defaults(ctx)
    # the other profiled instantiations
    for what, bt, pp, want in (
            ("Q rec", batch, icp_config.shipped_params(**tiers.P2P_REC), L.ICP_ROUTE_Q),
            ("LDS", _uniform_batch(ctx, ctx.n_cu + 8, 8000, 6000, 5200), p, L.ICP_ROUTE_LDS),
            ("T1", _uniform_batch(ctx, 16, 300, 1000, 5300), icp_config.shipped_params(), L.ICP_ROUTE_T1)):
        plain = outl._jobs(ctx, pp, None, *bt)
        assert (plain[3] == want).all(), (what, np.unique(plain[3]))
        got, c = _profiled(ctx, lambda: outl._jobs(ctx, pp, None, *bt))
        outl._same(got, plain, ("profiled", what))
        assert c[84] == int(plain[2].sum()), what


# ---- 6: the watchdog ----------------------------------------------------------------------------------------------

def test_no_watchdog_trips_at_the_extremes(ctx, batches, capfd):
    """icp_debug = 1 reports a loop that ran past its watchdog bound (SW_WATCH, the 20-round limit) on stderr; without
    it such a loop just stops.  STARVED and GENEROUS on both batches: nothing reported, and the results of the
    default run"""
    for name in ("mixed", "ties"):
        batch, _ = batches[name]
        for chain in ("p2p30", "shipped"):
            base = _call(ctx, chain, batch)
            for knobs in (STARVED, GENEROUS):
                capfd.readouterr()
                got = _call(ctx, chain, batch, icp_debug=1, **knobs)
                err = capfd.readouterr().err
                assert "sfe_icp_sweep: watchdog" not in err, (name, chain, _knob_id(knobs), err)
                _same(got, base, (name, chain, _knob_id(knobs), "debug"))
    _assert_defaults(ctx)
