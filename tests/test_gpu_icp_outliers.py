"""GPU: the outlier filters and the checker of ``sfe_icp_outliers`` inside the ICP loop (MinDist, MedianDist, Null,
Bound), on every route of the launcher.

Equivalences with the existing entry points, bit for bit (MedianDist{1} == TrimmedDist{0.5}; MinDist{0}, Null and a
Bound that is never reached == the chain without them); every route (tiny, one-wave, four-wave, the 1024-thread builds,
split jobs, brute force) against the numpy restatement (tests/icp_chain_ref.py: status and iterations equal, pose
within 1e-6), each route asserted with ``Context.icp_routes``; distances exactly on minDist^2 and on factor x median
and one ulp either side; the Bound checker's status and its place among the checkers; and a median filter on a job
without a finite distance."""
import numpy as np
import pytest

from sonar_slam_amd import _lib as L
from sonar_slam_amd import icp_config, pcl, synth

import icp_chain_ref

pytestmark = pytest.mark.gpu

TOL_TIGHT = 1e-6
ONE_SIZE = dict(sw_tiers=0, sw_multi=0, sw_tiny=0)


def _pose_diff(Ta, Tb):
    a, b = synth.pose_of(Ta), synth.pose_of(Tb)
    return max(abs(a[0] - b[0]), abs(a[1] - b[1]), abs(np.arctan2(np.sin(a[2] - b[2]), np.cos(a[2] - b[2]))))


def _ox(**kw):
    return L.IcpOutliers(**kw)


def _icp(ctx, p, ox=None):
    icp = pcl.ICP(ctx=ctx)
    icp.setChain(icp_config.IcpChain(p, outliers=ox))
    return icp


def _with_variant(ctx, variant, fn):
    ctx._check(ctx.lib.sfe_icp_set_tuning(ctx.handle, variant))
    try:
        return fn()
    finally:
        ctx._check(ctx.lib.sfe_icp_set_tuning(ctx.handle, 0))


def _pool(clouds):
    off = np.zeros(len(clouds) + 1, np.int64)
    off[1:] = np.cumsum([len(c) for c in clouds])
    return np.ascontiguousarray(np.concatenate(clouds), np.float32), off


def _jobs(ctx, p, ox, srcs, tgts, jobs, gs, variant=0, **knobs):
    """one compute_jobs call -> (status, T, iters, routes)"""
    sp, so = _pool(srcs)
    tp, to = _pool(tgts)
    j4 = np.array([(so[a], len(srcs[a]), to[b], len(tgts[b])) for a, b in jobs], np.int32)
    g9 = np.ascontiguousarray(np.stack(gs), np.float32).reshape(-1, 9)
    with ctx.tuning(**knobs):
        st, T, it = _with_variant(ctx, variant, lambda: _icp(ctx, p, ox).compute_jobs(sp, tp, j4, g9))
        routes = ctx.icp_routes(len(jobs))
    return st.copy(), T.copy(), it.copy(), routes


def _same(a, b, what):
    for k, name in enumerate(("status", "T", "iters")):
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, name, np.flatnonzero(
            (a[k] != b[k]).reshape(len(a[0]), -1).any(axis=1))[:10])


def _check_ref(p, ox, picks, srcs, tgts, jobs, gs, got, what):
    for j in picks:
        a, b = jobs[j]
        st, T, it = icp_chain_ref.icp(srcs[a], tgts[b], gs[j], p, ox)
        info = (what, j, len(srcs[a]), len(tgts[b]), int(got[3][j]))
        assert (int(got[0][j]), int(got[2][j])) == (st, it), info + (st, it)
        if st == 0:
            assert _pose_diff(got[1][j], T) < TOL_TIGHT, info + (_pose_diff(got[1][j], T),)
        else:
            assert np.array_equal(got[1][j], gs[j]), info


def _tile(pairs, n, rng, base=0):
    d = len(pairs)
    jobs = [(base + j % d, base + j % d) for j in range(n)]
    gs = [(pairs[j % d][2].astype(np.float64) @ synth.pose_matrix(*rng.normal(0, [0.05, 0.05, 0.005]))).astype(np.float32)
          for j in range(n)]
    return jobs, gs


def _batch(ctx, seed):
    """tiny, one-wave and four-wave jobs in a call of 2 x CUs small jobs (both small tiers live), and two 1024-thread jobs"""
    rng = np.random.default_rng(seed)
    sizes = [(int(a), int(b)) for a, b in zip(rng.integers(60, 300, 6), rng.integers(60, 300, 6))]       # tiny
    sizes += [(int(a), int(b)) for a, b in zip(rng.integers(330, 385, 6), rng.integers(400, 513, 6))]    # one wave
    n0 = len(sizes)
    sizes += [(int(a), int(b)) for a, b in zip(rng.integers(600, 1500, 4), rng.integers(513, 1500, 4))]  # four waves
    n_small = len(sizes)
    big = [(2600, 2600), (2200, 3000)]
    pairs = [synth.scan_pair(seed=seed + i, n_src=a, n_tgt=b) for i, (a, b) in enumerate(sizes + big)]
    srcs, tgts = [q[0] for q in pairs], [q[1] for q in pairs]
    n = 2 * ctx.n_cu + 64
    jobs, gs = _tile(pairs[:n0], 2 * ctx.n_cu, rng)
    j1, g1 = _tile(pairs[n0:n_small], n - 2 * ctx.n_cu, rng, base=n0)
    jobs += j1 + [(n_small + i, n_small + i) for i in range(len(big))]
    gs += g1 + [q[2] for q in pairs[n_small:]]
    return srcs, tgts, jobs, gs


def _route_picks(routes):
    """a few jobs of every route the call took"""
    picks = []
    for r in sorted(set(int(x) for x in routes)):
        picks += [int(j) for j in np.flatnonzero(routes == r)[:2]]
    return picks


LONG = dict(max_iter=30, use_diff_checker=0)       # the clearance-record builds
CHAINS = {
    "median2_maxdist": (dict(use_trimmed_filter=0), dict(use_median=1, median_factor=2.0)),
    "median3_trimmed_maxdist": ({}, dict(use_median=1, median_factor=3.0)),
    "median3_only_long": (dict(use_trimmed_filter=0, use_max_dist_filter=0, **LONG), dict(use_median=1, median_factor=3.0)),
    "median_half_maxdist": (dict(use_trimmed_filter=0, **LONG), dict(use_median=1, median_factor=0.5)),
    "mindist_only": (dict(use_trimmed_filter=0, use_max_dist_filter=0), dict(use_min_dist=1, min_dist=0.02)),
    "mindist_trimmed_maxdist": (LONG, dict(use_min_dist=1, min_dist=0.02)),
    "p2plane_median2_mindist": (dict(minimizer=1, use_trimmed_filter=0), dict(use_median=1, median_factor=2.0,
                                                                               use_min_dist=1, min_dist=0.01)),
    "p2plane_median3_trimmed": (dict(minimizer=1, **LONG), dict(use_median=1, median_factor=3.0)),
}


@pytest.fixture(scope="module")
def batch(ctx):
    return _batch(ctx, 4100)


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_every_route_against_the_restatement(ctx, batch, name):
    """the batch by default and with the tiny kernel off (on a short chain the one-wave jobs go to the tiny kernel):
    tiny, one-wave, four-wave and 1024-thread jobs, a few of each against the restatement; each run bit for bit equal to
    the same batch on the 1024-thread build and the picks to the brute-force kernel"""
    over, oxkw = CHAINS[name]
    p, ox = icp_config.shipped_params(**over), _ox(**oxkw)
    srcs, tgts, jobs, gs = batch
    n = 2 * ctx.n_cu + 64
    seen = set()
    one = _jobs(ctx, p, ox, srcs, tgts, jobs, gs, **ONE_SIZE)
    for knobs in ({}, dict(sw_tiny=0)):
        got = _jobs(ctx, p, ox, srcs, tgts, jobs, gs, **knobs)
        routes = got[3]
        assert set(int(x) for x in routes[n:]) <= {L.ICP_ROUTE_Q, L.ICP_ROUTE_LDS}, routes[n:]
        seen |= set(int(x) for x in routes)
        picks = sorted(set(_route_picks(routes) + [n - 1, len(jobs) - 1]))
        _check_ref(p, ox, picks, srcs, tgts, jobs, gs, got, (name, knobs))
        # every build sums in the order of a 1024-thread workgroup: the one-size run is the same bit for bit
        _same(got, one, (name, knobs, "one-size"))
    assert {L.ICP_ROUTE_TINY, L.ICP_ROUTE_T0, L.ICP_ROUTE_T1, L.ICP_ROUTE_Q} <= seen, (name, seen)
    # brute force (tuning bit 2)
    sub = sorted(set(range(0, len(jobs), 37)) | {len(jobs) - 1})
    brute = _jobs(ctx, p, ox, srcs, tgts, [jobs[j] for j in sub], [gs[j] for j in sub], variant=4)
    assert (brute[3] == L.ICP_ROUTE_BRUTE).all()
    _same(brute[:3], tuple(x[sub] for x in one[:3]), (name, "brute"))


@pytest.mark.parametrize("name", ["median3_trimmed_maxdist", "median_half_maxdist", "p2plane_median2_mindist"])
def test_split_jobs_against_the_restatement(ctx, name):
    """jobs shared by several workgroups (a target beyond the LDS limit): the median's order statistic and the re-search
    of its cap go through the cross-workgroup exchange; same decisions as unsplit, pose against the restatement"""
    over, oxkw = CHAINS[name]
    over = dict(over, max_iter=8, use_diff_checker=0)
    p, ox = icp_config.shipped_params(**over), _ox(**oxkw)
    src, tgt, guess, _ = synth.scan_pair(seed=77, n_src=4400, n_tgt=4600)
    src[::41] += 30.0
    big_t = np.concatenate([tgt, tgt + np.float32(0.013)]).astype(np.float32)     # 9200 > the LDS target limit
    gs = [guess, (guess.astype(np.float64) @ synth.pose_matrix(0.1, -0.05, 0.01)).astype(np.float32)]
    jobs = [(0, 0), (0, 0)]
    with ctx.tuning(sw_multi_min_src=4096, sw_multi_share_min=64):
        got = _jobs(ctx, p, ox, [src], [big_t], jobs, gs, sw_multi=1, sw_tiers=1)
        ref = _jobs(ctx, p, ox, [src], [big_t], jobs, gs, sw_multi=0)
    assert (got[3] == L.ICP_ROUTE_SPLIT).all(), got[3]
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2])
    assert max(_pose_diff(x, y) for x, y in zip(got[1], ref[1])) < TOL_TIGHT
    _check_ref(p, ox, [1], [src], [big_t], jobs, gs, got, name)


def test_equivalences_bit_for_bit(ctx, batch):
    """MedianDist{factor: 1} == TrimmedDist{ratio: 0.5}; MinDist{0} + Null + a Bound never reached == the chain without
    them, on every route and on brute force"""
    srcs, tgts, jobs, gs = batch
    for variant in (0, 4):
        sub = list(range(len(jobs))) if variant == 0 else list(range(0, len(jobs), 9))
        js, g = [jobs[j] for j in sub], [gs[j] for j in sub]
        trim = _jobs(ctx, icp_config.shipped_params(trim_ratio=0.5), None, srcs, tgts, js, g, variant)
        med = _jobs(ctx, icp_config.shipped_params(use_trimmed_filter=0), _ox(use_median=1, median_factor=1.0),
                    srcs, tgts, js, g, variant)
        _same(trim, med, ("median1", variant))
        assert np.array_equal(trim[3], med[3])
        for over in ({}, dict(minimizer=1, **LONG)):
            p = icp_config.shipped_params(**over)
            base = _jobs(ctx, p, None, srcs, tgts, js, g, variant)
            ch = icp_config.parse_icp_chain(
                "outlierFilters:\n  - MinDistOutlierFilter:\n      minDist: 0\n  - NullOutlierFilter\n"
                "transformationCheckers:\n  - BoundTransformationChecker:\n      maxRotationNorm: 3.0\n"
                "      maxTranslationNorm: 1000\n")
            assert ch.outliers.use_min_dist and ch.outliers.use_bound
            got = _jobs(ctx, p, ch.outliers, srcs, tgts, js, g, variant)
            _same(base, got, ("neutral", over, variant))


def _nx(a, toward):
    return np.nextafter(np.float32(a), np.float32(toward), dtype=np.float32)


D, M2 = np.float32(0.0625), np.float32(0.125)       # the median of the pairs below, and twice it


def _threshold_pair():
    """a 9 x 9 grid target (spacing 2, mean exactly 0: centring changes no coordinate) and a source whose d2 are exact:
    15 pairs at 1/64, 45 at D = 1/16 (the median of the 81), one each one ulp below and above D, one each at 2 D and one
    ulp either side of it, 16 at 1/4 (every sum and product below is exact in float, or rounds as stated)"""
    g = np.stack(np.meshgrid(np.arange(-8, 9, 2.0), np.arange(-8, 9, 2.0)), -1).reshape(-1, 2).astype(np.float32)
    special = {(0, 0): (_nx(0.25, 0), 2.0 ** -14),      # fl(0.25^-)^2 = D - 2 ulp, + 2^-28: D - 1 ulp
               (2, 0): (0.25, 2.0 ** -13.75),          # D + fl(dy^2) (between 1/2 and 3/2 ulp): D + 1 ulp
               (4, 0): (0.25, 0.0),                    # D
               (6, 0): (0.25, 0.25),                   # 2 D
               (8, 0): (0.25, _nx(0.25, 1)),           # 2 D + 1 ulp
               (-2, 0): (0.25, _nx(0.25, 0))}          # 2 D - 1 ulp
    rest = [(0.125, 0.0)] * 15 + [(0.25, 0.0)] * 44 + [(0.5, 0.0)] * 16
    off, k = [], 0
    for x, y in g:
        if (int(x), int(y)) in special:
            off.append(special[(int(x), int(y))])
        else:
            off.append(rest[k])
            k += 1
    src = (g.astype(np.float64) + np.array(off, np.float64)).astype(np.float32)
    d = (src[:, 0] - g[:, 0]) ** 2 + (src[:, 1] - g[:, 1]) ** 2
    d2 = np.float32(src[:, 0] - g[:, 0]) ** 2 + np.float32(src[:, 1] - g[:, 1]) ** 2
    for want in (_nx(D, 0), D, _nx(D, 1), _nx(M2, 0), M2, _nx(M2, 1)):
        assert (d2 == want).sum() >= 1, want
    assert np.float32(np.sort(d2)[int(np.float32(len(d2)) * np.float32(0.5))]) == D and len(d) == 81
    return src, g


@pytest.mark.parametrize("knobs, variant", [({}, 0), (ONE_SIZE, 0), ({}, 4)])
def test_thresholds_one_ulp_either_side(ctx, knobs, variant):
    """matches at d2 = minDist^2 (kept) and one ulp either side, and at factor x median (kept) and one ulp either side:
    minDist^2 = D - 2 ulp / D / D + 2 ulp keeps 3 / 2 / 0 of the three pairs around D, factor 2^- / 2 / 2^+ keeps 1 / 2 / 3
    of those around 2 D -- each of the six chains a different pose, every one equal to the restatement's"""
    src, tgt = _threshold_pair()
    guess = np.eye(3, dtype=np.float32)
    p = icp_config.shipped_params(use_max_dist_filter=0, use_trimmed_filter=0, max_iter=1, use_diff_checker=0)
    mins = [_nx(0.25, 0), np.float32(0.25), _nx(0.25, 1)]
    assert [np.float32(m * m) for m in mins] == [_nx(_nx(D, 0), 0), D, _nx(_nx(D, 1), 1)]
    cases = [_ox(use_min_dist=1, min_dist=float(m)) for m in mins]
    cases += [_ox(use_median=1, median_factor=float(f)) for f in (_nx(2, 0), 2.0, _nx(2, 4))]
    poses = []
    for ox in cases:
        got = _jobs(ctx, p, ox, [src], [tgt], [(0, 0)], [guess], variant, **knobs)
        _check_ref(p, ox, [0], [src], [tgt], [(0, 0)], [guess], got, ("threshold", knobs, variant, ox))
        assert int(got[0][0]) == 0
        poses.append(got[1][0])
    for i in range(len(poses)):
        for j in range(i):
            assert not np.array_equal(poses[i], poses[j]), (i, j)


def test_median_without_a_finite_distance(ctx):
    src, tgt, guess, _ = synth.scan_pair(seed=5, n_src=300, n_tgt=300)
    far = src + np.float32(500.0)
    p = icp_config.shipped_params(use_trimmed_filter=0)
    for variant in (0, 4):
        st, T, it, _ = _jobs(ctx, p, _ox(use_median=1, median_factor=3.0), [far], [tgt], [(0, 0)], [guess], variant)
        assert (int(st[0]), int(it[0])) == (1, 0) and np.array_equal(T[0], guess)
        assert L.ICP_STATUS_MESSAGES[int(st[0])] == "no outlier to filter"


def test_median_when_every_distance_is_zero(ctx):
    """The median is taken over the finite distances, a distance of 0 included -- as the trimmed quantile here (and
    the oracle) take theirs; libpointmatcher's getDistsQuantile counts only d2 > 0, where this job would report status 1.
    A source equal to its target: every d2 is 0, so is the median, and the limit 0 keeps every pair (status 0), the same
    bits as TrimmedDist{0.5}."""
    _, tgt, _, _ = synth.scan_pair(seed=6, n_src=300, n_tgt=300)
    guess = np.eye(3, dtype=np.float32)
    p = icp_config.shipped_params(use_trimmed_filter=0, max_iter=3, use_diff_checker=0)
    ox = _ox(use_median=1, median_factor=3.0)
    for knobs, variant in (({}, 0), (ONE_SIZE, 0), ({}, 4)):
        got = _jobs(ctx, p, ox, [tgt], [tgt], [(0, 0)], [guess], variant, **knobs)
        assert int(got[0][0]) == 0, got[:3]
        _check_ref(p, ox, [0], [tgt], [tgt], [(0, 0)], [guess], got, ("zero", knobs, variant))
        trim = _jobs(ctx, icp_config.shipped_params(trim_ratio=0.5, max_iter=3, use_diff_checker=0), None, [tgt], [tgt],
                     [(0, 0)], [guess], variant, **knobs)
        _same(got, trim, ("zero vs trimmed", knobs, variant))


def _bound_case():
    src, tgt, guess, _ = synth.scan_pair(seed=12, n_src=400, n_tgt=450, guess_error=(0.6, -0.4, 0.05))
    return src, tgt, guess


def test_bound_stops_the_job(ctx):
    """guesses far enough off that T_iter's translation passes maxTranslationNorm: status 9, T = the guess bit for bit.
    The rotation limit stays far (radians apart) from acosf(T00): device acosf is not correctly rounded."""
    src, tgt, guess = _bound_case()
    p = icp_config.shipped_params()
    ox = _ox(use_bound=1, max_rotation_norm=1.0, max_translation_norm=0.2, bound_order=1)
    for knobs, variant in (({}, 0), (ONE_SIZE, 0), ({}, 4)):
        got = _jobs(ctx, p, ox, [src], [tgt], [(0, 0)], [guess], variant, **knobs)
        assert int(got[0][0]) == L.ICP_BOUND and np.array_equal(got[1][0], guess), got[:3]
        _check_ref(p, ox, [0], [src], [tgt], [(0, 0)], [guess], got, ("bound", knobs, variant))
        msg, T = _with_variant(ctx, variant, lambda: _icp(ctx, p, ox).compute(src, tgt, guess))
        assert msg == "limit out of bounds" and np.array_equal(T, guess)


def test_bound_listed_after_counter_skips_the_last_iteration(ctx):
    """the first iteration whose T_iter is out of bounds found by the restatement is made the Counter's last: listed
    after the Counter, Bound is not evaluated there (success); listed before it, the job is bounded"""
    src, tgt, guess = _bound_case()
    p = icp_config.shipped_params(use_diff_checker=0)
    first = _ox(use_bound=1, max_rotation_norm=1.0, max_translation_norm=0.6, bound_order=0)
    st, _, k = icp_chain_ref.icp(src, tgt, guess, p, first)
    assert st == L.ICP_BOUND and k >= 2          # (the limit is 0.5 % away from where T_iter passes it)
    p = icp_config.shipped_params(use_diff_checker=0, max_iter=k)
    after = _ox(use_bound=1, max_rotation_norm=1.0, max_translation_norm=0.6, bound_order=1)
    for knobs, variant in (({}, 0), (ONE_SIZE, 0), ({}, 4)):
        a = _jobs(ctx, p, after, [src], [tgt], [(0, 0)], [guess], variant, **knobs)
        b = _jobs(ctx, p, first, [src], [tgt], [(0, 0)], [guess], variant, **knobs)
        assert (int(a[0][0]), int(a[2][0])) == (0, k), a[:3]
        assert (int(b[0][0]), int(b[2][0])) == (L.ICP_BOUND, k), b[:3]
        _check_ref(p, after, [0], [src], [tgt], [(0, 0)], [guess], a, ("after", variant))
        _check_ref(p, first, [0], [src], [tgt], [(0, 0)], [guess], b, ("first", variant))


def test_nothing_of_one_call_survives_into_the_next():
    """The outlier settings and the unsplit retry travel with the call, not on the context: after a ``*_chain_ext`` call
    with MedianDist that is refused with SFE_ERR_ARG (a job outside its pool), a plain ``sfe_icp_compute_jobs`` and a
    ``*_chain_ext`` call give bit for bit what the same calls give on a context that has seen nothing else"""
    p, ox = icp_config.shipped_params(use_trimmed_filter=0), _ox(use_median=1, median_factor=2.0)
    pairs = [synth.scan_pair(seed=5200 + i, n_src=a, n_tgt=b) for i, (a, b) in enumerate([(150, 180), (700, 900), (2600, 2600)])]
    srcs, tgts, gs = [q[0] for q in pairs], [q[1] for q in pairs], [q[2] for q in pairs]
    jobs = [(i, i) for i in range(len(pairs))]

    def calls(c):
        return [_jobs(c, p, o, srcs, tgts, jobs, gs)[:3] for o in (None, ox, None)]

    used, fresh = L.Context(0), L.Context(0)
    try:
        sp, tp = _pool(srcs)[0], _pool(tgts)[0]
        beyond = np.array([[0, len(sp) + 1, 0, len(tgts[0])]], np.int32)
        with pytest.raises(L.SonarFEError, match="libsonarfe error -1:"):
            _icp(used, p, ox).compute_jobs(sp, tp, beyond, np.asarray(gs[0], np.float32).reshape(1, 9))
        got, want = calls(used), calls(fresh)
    finally:
        used.close()
        fresh.close()
    for k, what in enumerate(("plain after the refused call", "chain_ext", "plain after chain_ext")):
        _same(got[k], want[k], what)
    _same(want[0], want[2], "plain twice")
    assert not np.array_equal(want[0][1], want[1][1]), "MedianDist{2} left every pose as it was: the chain_ext call shows nothing"
