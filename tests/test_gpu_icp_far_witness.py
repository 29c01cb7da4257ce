"""GPU: the two-level witness grid of the ICP target preparation (sweep_grid_witness, sfe_icp_sweep_prep.hip) and
the first iteration of the jobs that start from it.

The grid hands every query of the first iteration a real target point as an upper bound of its neighbour distance.  Its
fine level reaches four cells around the structures; a second, coarse level (one cell per 8 x 8 fine cells, dilated
until it is full) serves the fine cells that are still empty, so the scattered queries far from every wall start with
a bound too instead of scanning their whole maxDist box for one.  The search inside the bound is exact whatever the
witness is, so nothing a job computes may depend on the grid.

* The grid itself, read back from the preparation's scratch (generation 0), against the numpy restatement
  tests/icp_far_witness_ref.py: the grid's geometry and the claimed cells bit for bit on every build; the whole grid bit
  for bit on the one-wave build, whose in-place fine sweeps are deterministic; on the builds of several waves, where
  the order of the fine sweeps' evaluation is not, the properties: every witness is one of the claimed ones (a real,
  finite target point) and no cell is empty unless the target has no finite point.
* End to end: every case under 1, 3 and 30 iterations of both minimisers and under the shipped chain, on the builds a
  call of few jobs selects (the four-wave build: at most 320 queries, targets of at most 2048 points), on the
  1024-thread builds and, tiled to 2 x CUs + 16 jobs, on the one-wave build: bit for bit the brute-force kernel, status
  and iteration count those of the oracle in fp64-sum mode and the pose within 1e-6.  As in test_gpu_icp_sorts, targets
  with NaN points and clouds whose point-to-plane system is singular (one line, one point) are held against the
  brute-force kernel alone.

There is no switch for the second level: the tree has one grid."""
import ctypes as C

import numpy as np
import pytest

from sonar_slam_amd import _lib as L
from sonar_slam_amd import icp_config, synth

import icp_far_witness_ref as ref
import test_gpu_icp_sorts as sorts

pytestmark = pytest.mark.gpu

PAD = 68                                                    # SW_PAD (sfe_icp_sweep.h)
SLOT_STGT, SLOT_MEAN, SLOT_TAB, SLOT_GRID = 14, 17, 23, 38  # generation 0 of the preparation's scratch (sfe_icp_sweep.hip)
TAB_WORDS = 12 + 65 + 64 + 64                               # StripTab
MAX_DIST2 = np.float32(100.0)                               # matcher_max_dist = 10 m
CHAINS = dict([("%s%d" % (("p2p", "p2plane")[m], it), dict(minimizer=m, max_iter=it, use_diff_checker=0))
               for m in (0, 1) for it in (1, 3, 30)] + [("shipped", {})])
# build -> (knobs, grid cells of its preparation)
BUILDS = {"four waves": (sorts.NO_TINY, 2048), "1024": (sorts.ONE_SIZE, 8192)}
GM_ONE_WAVE = 512


# ---- clouds -----------------------------------------------------------------------------------------------------

def _blob(rng, n, cx, cy, half=0.5):
    return np.c_[rng.uniform(cx - half, cx + half, n), rng.uniform(cy - half, cy + half, n)]


def _case(name):
    """-> (source, target, guess, whether the oracle can judge the case)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    g = sorts._guess(rng)
    if name == "gap":            # two clusters 8 m apart, a fifth of the queries between them: witnesses of the coarse level only
        tgt = np.r_[_blob(rng, 150, -4.5, 0.0), _blob(rng, 150, 4.5, 0.0)].astype(np.float32)
        src = np.r_[sorts._moved(rng, tgt, 240), np.c_[rng.uniform(-2.5, 2.5, 60), rng.uniform(-0.4, 0.4, 60)].astype(np.float32)]
        return src, tgt, g, True
    if name == "far":            # a tenth of the queries more than maxDist from every target, on all sides: they end `none`
        tgt = np.r_[_blob(rng, 200, 0.0, 0.0, 3.0), _blob(rng, 100, 5.0, 2.0)].astype(np.float32)
        th = rng.uniform(0, 2 * np.pi, 30)
        far = np.c_[np.cos(th), np.sin(th)] * rng.uniform(18, 30, 30)[:, None]
        return np.r_[sorts._moved(rng, tgt, 270), far.astype(np.float32)], tgt, g, True
    if name in ("n1", "n2", "n3", "n65"):
        n = int(name[1:])
        src, tgt, g, _ = synth.scan_pair(seed=6100 + n, n_src=max(n, 40), n_tgt=n)
        return src, tgt, g, n > 3
    if name == "identical":      # a box of zero extent: one cell
        tgt = np.repeat(np.array([[1.25, -0.5]], np.float32), 40, axis=0)
        return (tgt[0] + rng.normal(0, [2.0, 2.0], (60, 2))).astype(np.float32), tgt, g, False
    if name == "line":           # a box of zero height: the cell count of 4097 x 1 is halved on the smaller builds
        tgt = sorts._on_a_line(rng, 150)
        return np.r_[sorts._moved(rng, tgt, 130), _blob(rng, 20, 0.0, 6.0, 4.0).astype(np.float32)], tgt, g, False
    if name == "gm":             # 1023 : 1 and at least half as many points as the four-wave grid has cells: 1024 x 2 cells
        tgt = np.c_[rng.uniform(-20.46, 20.46, 1100), rng.uniform(-0.02, 0.02, 1100)]
        tgt[:4] = [(-20.46, 0.0), (20.46, 0.0), (0.0, -0.02), (0.0, 0.02)]
        tgt = tgt.astype(np.float32)
        return np.r_[sorts._moved(rng, tgt, 280), _blob(rng, 20, 0.0, 5.0, 3.0).astype(np.float32)], tgt, g, False
    if name == "nan":            # NaN coordinates in both clouds
        src, tgt, g, _ = synth.scan_pair(seed=6200, n_src=300, n_tgt=400)
        src, tgt = src.copy(), tgt.copy()
        src[rng.integers(0, 300, 3), 0] = np.nan
        src[rng.integers(0, 300, 3), 1] = np.nan
        tgt[rng.integers(0, 400, 3), 0] = np.nan
        tgt[rng.integers(0, 400, 3), 1] = np.nan
        return src, tgt, g, False
    if name == "union":          # one query in a 6 m hole of a wall, its neighbours in the sorted order on the wall
        x = np.r_[rng.uniform(-10, -1, 220), rng.uniform(5, 8, 80)]
        tgt = np.c_[x, rng.normal(0, 0.03, 300)].astype(np.float32)
        src = sorts._moved(rng, tgt, 299)
        Tg = g.astype(np.float64)
        hole = np.linalg.solve(Tg[:2, :2], np.array([2.0, 0.0]) - Tg[:2, 2])         # lands at (2, 0) under the guess
        return np.r_[src, hole[None].astype(np.float32)], tgt, g, True
    if name == "scan":           # a sonar-like pair with scattered outliers
        src, tgt, g, _ = synth.scan_pair(seed=6300, n_src=320, n_tgt=500)
        return src, tgt, g, True
    raise KeyError(name)


CASES = ["gap", "far", "n1", "n2", "n3", "n65", "identical", "line", "gm", "nan", "union", "scan"]


# ---- the grid, read back ------------------------------------------------------------------------------------------

def _scratch(ctx, slot, dtype, n):
    out = np.empty(n, dtype)
    ctx._check(ctx.lib.sfe_debug_read_scratch(ctx.handle, slot, out.ctypes.data_as(C.c_void_p), out.nbytes))
    return out


def _prepared(ctx, nt):
    """the first (only) prepared target of the last call -> (S, geometry, grid, mean)"""
    tab = _scratch(ctx, SLOT_TAB, np.int32, TAB_WORDS)
    f = tab.view(np.float32)
    ln = int(tab[1])
    assert nt + 2 <= ln <= nt + PAD - 3, (ln, nt)
    geo = dict(gx0=f[5], gy0=f[6], ginv=f[7], gnx=int(tab[8]), gny=int(tab[9]))
    S = _scratch(ctx, SLOT_STGT, np.float32, 2 * (nt + PAD)).reshape(-1, 2)[:ln + 2]
    grid = _scratch(ctx, SLOT_GRID, np.int32, geo["gnx"] * geo["gny"]).astype(np.int64)
    return S, geo, grid, _scratch(ctx, SLOT_MEAN, np.float32, 2)


def _one_wave_jobs(ctx, pairs, rng):
    """2 x CUs + 16 jobs over the pairs, the first of every pair with its own guess -> (jobs, guesses)"""
    n = 2 * ctx.n_cu + 16
    d = len(pairs)
    jobs = [(j % d, j % d) for j in range(n)]
    gs = [pairs[j][2] if j < d else
          (pairs[j % d][2].astype(np.float64) @ synth.pose_matrix(*rng.normal(0, [0.05, 0.05, 0.005]))).astype(np.float32)
          for j in range(n)]
    return jobs, gs


def _prepare(ctx, build, src, tgt, g):
    """one iteration on `build` -> what its preparation left"""
    p = icp_config.shipped_params(minimizer=1, max_iter=1, use_diff_checker=0)
    if build == "one wave":
        jobs, gs = _one_wave_jobs(ctx, [(src, tgt, g)], np.random.default_rng(1))
        got = sorts._run(ctx, p, [src], [tgt], jobs, gs, **sorts.NO_TINY)
        assert (got[3] == L.ICP_ROUTE_T0).all(), np.unique(got[3])
    else:
        got = sorts._run(ctx, p, [src], [tgt], [(0, 0)], [g], **BUILDS[build][0])
        want = {L.ICP_ROUTE_T1} if build == "four waves" else {L.ICP_ROUTE_Q, L.ICP_ROUTE_LDS}
        assert set(got[3]) <= want, (build, got[3])
    return _prepared(ctx, len(tgt))


def _check_grid(S, geo, grid, nt, gm, exact, what):
    """-> the restatement's (final grid, claimed cells, fine level after synchronous / exact sweeps, coarse level)"""
    want_geo = ref.geometry(S, nt, gm)
    assert geo == want_geo, (what, geo, want_geo)
    out = ref.two_level(S, geo, chunk=64 if exact else None)
    final, claimed = out[0], out[1]
    finite = np.flatnonzero(np.isfinite(S).all(axis=1))
    assert np.array_equal(grid[claimed != 0], claimed[claimed != 0]), (what, "claimed cells")
    if len(finite) == 0:
        assert not grid.any(), what
        return out
    assert np.isin(grid, claimed[claimed != 0]).all(), (what, "a witness nobody claimed", np.flatnonzero(~np.isin(grid, claimed))[:10])
    assert np.isin(grid, finite).all() and (grid != 0).all(), (what, "empty cells", np.flatnonzero(grid == 0)[:10])
    assert (final != 0).all(), what
    if exact:
        assert np.array_equal(grid, final), (what, np.flatnonzero(grid != final)[:10])
    return out


GRID_CASES = [(n, b) for n in ("gap", "far", "n1", "n3", "n65", "identical", "line", "gm", "nan", "scan")
              for b in ("one wave", "four waves", "1024") if (n, b) != ("gm", "one wave")]   # (at most 512 points there)


@pytest.mark.parametrize("name,build", GRID_CASES)
def test_grid_against_the_restatement(ctx, name, build):
    src, tgt, g, _ = _case(name)
    S, geo, grid, _ = _prepare(ctx, build, src, tgt, g)
    gm = GM_ONE_WAVE if build == "one wave" else BUILDS[build][1]
    final, claimed, fine, level = _check_grid(S, geo, grid, len(tgt), gm, build == "one wave", (name, build))
    ncell = geo["gnx"] * geo["gny"]
    if name == "identical":
        assert ncell == 1 and grid[0] != 0
    if name == "line":
        assert (geo["gnx"], geo["gny"]) == ({"one wave": 257, "four waves": 1025, "1024": 4097}[build], 1)
        assert level[0] == (5 if build == "1024" else 3)    # 4097 cells in a row: coarse cells of 32 fine ones
    if name == "gm" and build == "four waves":
        assert (geo["gnx"], geo["gny"]) == (1024, 2) and ncell == gm
    if name == "nan":                                       # (a NaN mean: no finite centred point, an empty grid)
        assert not grid.any()
    if name == "gap":
        # the queries between the clusters stand in cells the fine sweeps do not reach (restated synchronously: what
        # every order fills at least; exactly on the one-wave build) -- and hold a witness all the same
        q = (src.astype(np.float64) @ g[:2, :2].T.astype(np.float64) + g[:2, 2].astype(np.float64)).astype(np.float32)
        mean = (tgt.astype(np.float64).sum(0) / len(tgt)).astype(np.float32)
        qc = ref.cell_of(q[240:, 0] - mean[0], q[240:, 1] - mean[1], geo)
        assert (fine[qc] == 0).sum() >= (30 if build == "one wave" else 1), (build, (fine[qc] == 0).sum())
        assert (grid[qc] != 0).all()
        assert level[4] >= 1                                # the coarse level had empty cells of its own to fill


# ---- end to end ---------------------------------------------------------------------------------------------------

def _check(ctx, srcs, tgts, gs, what, with_oracle, jobs=None, builds=("four waves", "1024"), chains=None):
    """every chain on `builds`: bit for bit the brute-force kernel; status, iterations and pose those of the oracle
    (with_oracle: True = every job, a list = those jobs, False = none)"""
    jobs = jobs if jobs is not None else [(j, j) for j in range(len(srcs))]
    for chain in chains or CHAINS:
        p = icp_config.shipped_params(**CHAINS[chain])
        brute = sorts._run(ctx, p, srcs, tgts, jobs, gs, variant=4)
        assert (brute[3] == L.ICP_ROUTE_BRUTE).all()
        for build in builds:
            got = sorts._run(ctx, p, srcs, tgts, jobs, gs, **(sorts.NO_TINY if build == "one wave" else BUILDS[build][0]))
            small = {L.ICP_ROUTE_T0} if build == "one wave" else {L.ICP_ROUTE_T1}
            assert set(got[3]) <= ({L.ICP_ROUTE_Q, L.ICP_ROUTE_LDS} if build == "1024" else small), (what, chain, build, got[3])
            sorts._same(got, brute, (what, chain, build))
        if with_oracle:
            judged = list(range(len(jobs))) if with_oracle is True else with_oracle
            sorts._check_oracle(p, judged, srcs, tgts, jobs, gs, brute, (what, chain))


@pytest.mark.parametrize("name", CASES)
def test_cases_on_the_four_wave_and_1024_thread_builds(ctx, name):
    src, tgt, g, with_oracle = _case(name)
    assert len(src) <= 320 and len(tgt) <= 2048
    _check(ctx, [src], [tgt], [g], name, with_oracle)


def test_cases_on_the_one_wave_build(ctx):
    """the cases of at most 384 x 512 points, tiled to 2 x CUs + 16 jobs"""
    pairs = [_case(n) for n in CASES]
    pairs = [q for q in pairs if len(q[0]) <= 384 and len(q[1]) <= 512]
    assert len(pairs) >= 10
    jobs, gs = _one_wave_jobs(ctx, pairs, np.random.default_rng(61))
    judged = [j for j, q in enumerate(pairs) if q[3]]
    srcs, tgts = [q[0] for q in pairs], [q[1] for q in pairs]
    _check(ctx, srcs, tgts, gs, "one wave", judged, jobs=jobs, builds=("one wave",))


def test_eight_guesses_on_one_target(ctx):
    """one preparation, one grid, eight jobs"""
    rng = np.random.default_rng(62)
    src, tgt, g, _ = _case("gap")
    gs = [g] + [(g.astype(np.float64) @ synth.pose_matrix(*rng.normal(0, [0.1, 0.1, 0.01]))).astype(np.float32) for _ in range(7)]
    _check(ctx, [src], [tgt], gs, "eight guesses", True, jobs=[(0, 0)] * 8)


def _mirrored_clusters(rng):
    """two clusters 8 m apart on the 1/64 m lattice, mirrored about the origin: the mean is exactly 0, so centring
    moves no coordinate, and under the identity guess a query stands exactly where its source point is"""
    half = np.round(_blob(rng, 150, 4.5, 0.0) * 64) / 64
    return np.ascontiguousarray(np.r_[half, -half], np.float32)


def _at_max_dist(S, geo, grid):
    """three queries above the gap between the clusters (beyond the box: the top row's cell of their column) whose
    grid witness lies at maxDist^2 exactly, one ulp inside and one ulp outside -> (queries [3 x 2], the cell, witness)"""
    x0 = np.float32(0.125)
    c = int(ref.cell_of(x0, np.float32(9.0), geo))
    w = int(grid[c])
    t = S[w]
    dy = np.sqrt(100.0 - (float(x0) - float(t[0])) ** 2)
    want = [np.nextafter(MAX_DIST2, np.float32(0)), MAX_DIST2, np.nextafter(MAX_DIST2, np.float32(np.inf))]
    found = {}
    ys = np.float32(t[1] + dy) + np.arange(-8, 9).astype(np.float32) * np.float32(2.0 ** -20)
    xs = x0 + np.arange(-4096, 4097).astype(np.float32) * np.float32(2.0 ** -24)
    for y in ys:
        d = ref._dist2(xs, np.full_like(xs, y), np.full_like(xs, t[0]), np.full_like(xs, t[1]))
        for k, v in enumerate(want):
            hit = np.flatnonzero(d == v)
            if k not in found and len(hit):
                found[k] = (xs[hit[0]], y)
    assert len(found) == 3, found
    q = np.array([found[k] for k in range(3)], np.float32)
    assert (ref.cell_of(q[:, 0], q[:, 1], geo) == c).all()
    return q, c, w


@pytest.mark.parametrize("build", list(BUILDS))
def test_coarse_witness_at_max_dist(ctx, build):
    """A coarse witness at maxDist, one ulp inside (both are matches: the query is bounded by them) and one ulp outside
    (it settles nothing: the query is put off to the cooperative tier as before), next to nearer targets that only the
    search finds.  The queries are built from the grid that the build's own preparation leaves."""
    rng = np.random.default_rng(63)
    tgt = _mirrored_clusters(rng)
    eye = np.eye(3, dtype=np.float32)
    wall = (tgt[rng.integers(0, len(tgt), 200)] + rng.normal(0, 0.03, (200, 2))).astype(np.float32)
    S, geo, grid, mean = _prepare(ctx, build, wall, tgt, eye)
    assert mean.tolist() == [0.0, 0.0]
    _check_grid(S, geo, grid, len(tgt), BUILDS[build][1], False, ("max dist", build))
    q, c, w = _at_max_dist(S, geo, grid)
    P = S[np.isfinite(S).all(axis=1)]
    for k in range(3):
        d = ref._dist2(np.full(len(P), q[k, 0]), np.full(len(P), q[k, 1]), P[:, 0], P[:, 1])
        assert d.min() < np.float32(99.0), (k, d.min())     # a nearer target, well within maxDist
    src = np.ascontiguousarray(np.r_[wall, q], np.float32)
    _check(ctx, [src], [tgt], [eye], ("max dist", build), True, builds=(build,))
    S2, geo2, grid2, _ = _prepared(ctx, len(tgt))           # (the last run of _check: this build's)
    assert geo2 == geo and grid2[c] == w, "the preparation of the checked run left another witness"
