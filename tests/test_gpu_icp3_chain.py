"""GPU: ICP chains on N x 3 clouds (sfe_icp3_dpf.hip, the EXT build of icp3_job_kernel, the dims = 3 plumbing).

- The filter pass (sfe_icp3_filter_clouds_dev) against tests/dpf3_ref.py, bit for bit in points and counts: about 40 clouds
  per call at the sizes around a wave, a workgroup and a chunk, with empty clouds between full ones; every survivor pattern;
  every ``dim``; boxes inside and outside; thresholds one ulp either side; the full stage count with two octree stages.  The
  octree stage against ``pcl.downsample`` on the same cloud.
- Equivalences, bit for bit: a chain with filters against the plain call on clouds filtered beforehand; MedianDist{1}
  against TrimmedDist{0.5}; MinDist{0}, Null and an unreachable Bound against the plain call; ``chain_ext`` with nothing
  listed; ``CloudStore3.icp(chain)`` against ``pcl.ICP.compute_jobs``; both minimisers.
- Against tests/icp3_chain_ref.py: status and iterations equal, T within 1e-6 (the bound tests/test_gpu_icp3.py holds the
  3-D kernel to), at the lane-ownership edges, the tile edges, the lattice boundary case, the failure statuses and Bound.
- z = 0 clouds against the 2-D device path; sharing of the filtered clouds and of the normals."""
import ctypes as C

import numpy as np
import pytest

from sonar_slam_amd import _lib as L
from sonar_slam_amd import icp_config, pcl, store

import dpf3_ref as D
import icp3_cases as C3
import icp3_chain_cases as K
import icp3_chain_ref as R
import icp3_ref

pytestmark = pytest.mark.gpu

TOL_TIGHT = 1e-6        # tests/test_gpu_icp3.py's bound on the 3-D kernel's pose against the reference
f32 = np.float32
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)


def _nx(a, toward):
    return np.nextafter(f32(a), f32(toward), dtype=f32)


def _diff(Ta, Tb):
    return float(np.abs(np.asarray(Ta, np.float64) - np.asarray(Tb, np.float64)).max())


def filter3(ctx, clouds, stages, lead=0):
    """sfe_icp3_filter_clouds_dev on clouds uploaded back to back (behind ``lead`` unused points) -> (clouds, counts)"""
    clouds = [np.ascontiguousarray(c, f32).reshape(-1, 3) for c in clouds]
    off = np.zeros(len(clouds) + 1, np.int64)
    off[0] = lead
    off[1:] = lead + np.cumsum([len(c) for c in clouds])
    pts = np.concatenate([np.full((lead, 3), 7.0, f32)] + clouds + [np.zeros((1, 3), f32)])
    d_in, d_out = ctx.alloc(pts.nbytes), ctx.alloc(pts.nbytes)
    d_in.upload(pts)
    arr, n = icp_config.IcpChain.device_stages(stages)
    counts = np.full(len(clouds), -5, np.int32)
    with ctx.lock:
        ctx._check(ctx.lib.sfe_icp3_filter_clouds_dev(ctx.handle, arr, n, d_in.ptr, L.ptr(off, C.c_int64), len(clouds),
                                                      d_out.ptr, L.ptr(counts, C.c_int32)))
        assert (counts >= 0).all()
        total = int(counts.sum())
        flat = d_out.download(f32, 3 * total).reshape(-1, 3) if total else np.zeros((0, 3), f32)
    d_in.free()
    d_out.free()
    at = np.concatenate([[0], np.cumsum(counts)])
    return [flat[at[k]:at[k + 1]] for k in range(len(clouds))], counts


def _same_clouds(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, (k, g.shape, w.shape)
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), k


def _pattern_clouds():
    """about 40 clouds: every size with random points, and at the sizes around a wave, a workgroup and a chunk the survivor
    patterns of the stage x < 1 -- all, none, alternating, only the first, only the last -- with empty clouds between"""
    rng = np.random.default_rng(3)
    clouds = [rng.uniform(-3, 3, (n, 3)).astype(f32) for n in SIZES]
    for n in (65, 257, 1025, 4097):
        base = rng.uniform(-3, 3, (n, 3)).astype(f32)
        for pat in ("all", "none", "alt", "first", "last"):
            c = base.copy()
            keep = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "alt": np.arange(n) % 2 == 0,
                    "first": np.arange(n) == 0, "last": np.arange(n) == n - 1}[pat]
            c[:, 0] = np.where(keep, f32(0.5), f32(1.5))
            clouds.append(c)
            if pat in ("none", "first"):
                clouds.append(np.zeros((0, 3), f32))
    return clouds


def test_filter_pass_survivor_patterns_and_sizes(ctx):
    clouds = _pattern_clouds()
    assert 36 <= len(clouds) <= 44
    st = [D.max_dist(1.0, 0)]
    got, counts = filter3(ctx, clouds, st)
    _same_clouds(got, [D.apply(c, st) for c in clouds])
    assert sorted(set(counts[len(SIZES):].tolist()))[:2] == [0, 1] and 4097 in counts
    # the same call on clouds that do not begin at the buffer's first point, and with no stage at all (a copy)
    _same_clouds(filter3(ctx, clouds, st, lead=13)[0], got)
    _same_clouds(filter3(ctx, clouds, [], lead=5)[0], clouds)


@pytest.mark.parametrize("name", ["dims", "norm", "boxes", "fused"])
def test_filter_pass_predicates(ctx, name):
    rng = np.random.default_rng(4)
    clouds = [rng.uniform(-3, 3, (n, 3)).astype(f32) for n in SIZES] + [np.zeros((0, 3), f32)]
    nonfinite = rng.uniform(-3, 3, (300, 3)).astype(f32)
    nonfinite[::7, 0], nonfinite[3::11, 1], nonfinite[5::13, 2] = np.nan, np.inf, -np.inf
    clouds.append(nonfinite)
    lo, hi = (-1.0, -2.0, -0.5), (2.0, 1.5, 2.5)
    lists = {"dims": [[D.max_dist(0.7, d)] for d in (0, 1, 2)] + [[D.min_dist(-0.9, d)] for d in (0, 1, 2)],
             "norm": [[D.max_dist(2.5)], [D.min_dist(2.5)], [D.max_dist(-2.5), D.min_dist(1.0)]],
             "boxes": [[D.box(lo, hi, 0)], [D.box(lo, hi, 1)]],
             "fused": [[D.max_dist(4.0), D.min_dist(0.2, 2), D.box(lo, hi, 0), D.max_dist(1.9, 0)],
                       [D.min_dist(0.4, 1), D.box(lo, hi, 1), D.max_dist(2.0, 2)]]}[name]
    for st in lists:
        got, _ = filter3(ctx, clouds, st)
        _same_clouds(got, [D.apply(c, st) for c in clouds])


def test_filter_pass_thresholds_one_ulp_either_side(ctx):
    thr = f32(1.7)
    xs = np.array([_nx(thr, -9), thr, _nx(thr, 9), _nx(-thr, -9), -thr, _nx(-thr, 9)], f32)
    for dim in (0, 1, 2):
        c = np.tile(np.array([0.3, -0.2, 0.1], f32), (len(xs), 1))
        c[:, dim] = xs
        for st in ([D.max_dist(thr, dim)], [D.min_dist(thr, dim)], [D.max_dist(-thr, dim)]):
            got, counts = filter3(ctx, [c, c[::-1].copy()], st)
            _same_clouds(got, [D.apply(c, st), D.apply(c[::-1], st)])
            assert 0 < counts[0] < len(xs)
    # the norm: (1.5, 2, 0) has norm 2.5 exactly; a box face through a coordinate
    c = np.array([[1.5, 2.0, 0.0], [0.0, 1.5, 2.0], [2.0, 0.0, -1.5], [_nx(1.5, 9), 2.0, 0.0], [_nx(1.5, 0), 2.0, 0.0]], f32)
    for t in (_nx(2.5, 0), f32(2.5), _nx(2.5, 9)):
        for st in ([D.max_dist(t)], [D.min_dist(t)]):
            _same_clouds(filter3(ctx, [c], st)[0], [D.apply(c, st)])
    lo, hi = (f32(-1.25), f32(-2.5), f32(0.5)), (f32(3.0), f32(-0.75), f32(4.5))
    pts = []
    for a in range(3):
        for face in (lo[a], hi[a]):
            for v in (_nx(face, -9), face, _nx(face, 9)):
                p = [f32(0.5), f32(-1.5), f32(2.0)]
                p[a] = v
                pts.append(p)
    c = np.array(pts, f32)
    for ri in (0, 1):
        got, counts = filter3(ctx, [c], [D.box(lo, hi, ri)])
        _same_clouds(got, [D.apply(c, [D.box(lo, hi, ri)])])
        assert counts[0] == (6 if ri == 0 else 12)


def _ds(ctx):
    return lambda p, size: pcl.downsample(p, size, ctx=ctx)


def test_octree_stage_is_pcl_downsample(ctx):
    rng = np.random.default_rng(6)
    clouds = [rng.uniform(-3, 3, (n, 3)).astype(f32) for n in (1, 2, 65, 257, 1025, 4097)]
    clouds.append(np.tile(np.array([[0.25, -1.5, 2.0]], f32), (300, 1)))                       # coincident points
    deep = np.concatenate([rng.uniform(0, 1e-5, (200, 3)), np.array([[1e6, -1e6, 1e6], [-1e6, 1e6, -1e6]])]).astype(f32)
    clouds += [deep, np.zeros((0, 3), f32)]                                                   # > 21 levels at size 1e-6
    for size in (0.5, 1e-6):
        got, counts = filter3(ctx, clouds, [D.octree(size)])
        for c, g in zip(clouds, got):
            want = pcl.downsample(c, size, ctx=ctx) if len(c) else c
            assert g.shape == want.shape and np.array_equal(g.view(np.uint32), want.view(np.uint32)), (size, len(c))
        assert counts[6] == 1 and counts[8] == 0
    # ... and the host restatement on the small ones
    got, _ = filter3(ctx, clouds[:4], [D.octree(0.5)])
    _same_clouds(got, [D.apply(c, [D.octree(0.5)]) for c in clouds[:4]])


def test_filter_pass_full_stage_count_with_two_octrees(ctx):
    rng = np.random.default_rng(7)
    st = [D.max_dist(6.0), D.octree(0.5), D.min_dist(0.1, 0), D.box((-2.5, -2.5, -2.5), (2.5, 2.5, 2.5), 0), D.octree(1.0),
          D.max_dist(2.0, 2), D.min_dist(0.3), D.box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5), 1)]
    assert len(st) == L.DPF_MAX_STAGES
    clouds = [rng.uniform(-3, 3, (n, 3)).astype(f32) for n in (0, 1, 64, 257, 0, 1025, 4097, 300)]
    got, counts = filter3(ctx, clouds, st, lead=3)
    _same_clouds(got, [D.apply(c, st, _ds(ctx)) for c in clouds])
    assert counts[6] > 20
    # an octree stage first and last
    st = [D.octree(0.7), D.max_dist(1.0, 1), D.octree(1.4)]
    _same_clouds(filter3(ctx, clouds, st, lead=3)[0], [D.apply(c, st, _ds(ctx)) for c in clouds])


def test_argument_errors_come_before_any_launch(ctx):
    src, tgt, g = K.pair(31, 50, 60)
    icp = pcl.ICP(ctx)
    bad = [[D.max_dist(1.0, 3)], [D.min_dist(1.0, -2)], [D.octree(0.0)], [D.octree(-1.0)], [D.stage(9)],
           [D.max_dist(9.0)] * (L.DPF_MAX_STAGES + 1)]
    for st in bad:
        icp.setChain(K.chain3(icp_config.shipped_params(), reference=st))
        with pytest.raises(RuntimeError):
            icp.compute(src, tgt, g)
        with pytest.raises(RuntimeError):
            filter3(ctx, [src], st)
    icp.setChain(K.chain3(icp_config.shipped_params(), use_median=1, median_factor=-1.0))
    with pytest.raises(RuntimeError):
        icp.compute(src, tgt, g)


# ---- equivalences, bit for bit ----------------------------------------------------------------------------------------------
def _jobs(ctx, chain_or_params, src, tgt, jobs4, g):
    icp = pcl.ICP(ctx)
    if isinstance(chain_or_params, icp_config.IcpChain):
        icp.setChain(chain_or_params)
    else:
        icp.setParams(chain_or_params)
    return icp.compute_jobs(src, tgt, np.asarray(jobs4, np.int32), np.asarray(g, f32).reshape(-1, 16))


def _same(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]), (a[0], b[0], a[2], b[2])
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def _pools(seed=41):
    """two pools of three clouds each and a job table that shares them"""
    a, b, c = K.pair(seed, 700, 900), K.pair(seed + 1, 300, 1100), K.pair(seed + 2, 1200, 500)
    srcs, tgts = [a[0], b[0], c[0]], [a[1], b[1], c[1]]
    so = np.concatenate([[0], np.cumsum([len(s) for s in srcs])])
    to = np.concatenate([[0], np.cumsum([len(t) for t in tgts])])
    pick = [(0, 0, a[2]), (1, 1, b[2]), (2, 2, c[2]), (0, 0, C3.GUESS.astype(f32)), (1, 1, b[2])]
    jobs4 = [[so[i], len(srcs[i]), to[j], len(tgts[j])] for i, j, _ in pick]
    return srcs, tgts, np.asarray(jobs4, np.int32), np.stack([g for _, _, g in pick]).astype(f32), pick


@pytest.mark.parametrize("minimizer", [0, 2])
def test_chain_with_filters_is_the_plain_call_on_filtered_clouds(ctx, minimizer):
    srcs, tgts, jobs4, g, pick = _pools()
    rd = [D.max_dist(3.2), D.min_dist(0.05, 2)]
    rf = [D.box((-2.8, -2.8, -1.9), (2.8, 2.8, 1.9), 0), D.octree(0.12)]
    p = icp_config.shipped_params(minimizer=minimizer)
    got = _jobs(ctx, K.chain3(p, rd, rf), np.concatenate(srcs), np.concatenate(tgts), jobs4, g)
    fs, ft = filter3(ctx, srcs, rd)[0], filter3(ctx, tgts, rf)[0]
    assert all(0 < len(f) < len(c) for f, c in zip(fs + ft, srcs + tgts))
    so = np.concatenate([[0], np.cumsum([len(s) for s in fs])])
    to = np.concatenate([[0], np.cumsum([len(t) for t in ft])])
    j2 = [[so[i], len(fs[i]), to[j], len(ft[j])] for i, j, _ in pick]
    want = _jobs(ctx, p, np.concatenate(fs), np.concatenate(ft), j2, g)
    _same(got, want)
    assert (got[0] == 0).all()
    # one side only
    got = _jobs(ctx, K.chain3(p, reference=rf), np.concatenate(srcs), np.concatenate(tgts), jobs4, g)
    j3 = [[jobs4[k][0], jobs4[k][1], to[j], len(ft[j])] for k, (i, j, _) in enumerate(pick)]
    _same(got, _jobs(ctx, p, np.concatenate(srcs), np.concatenate(ft), j3, g))


SHIPPED_WITH_NULL = """
matcher:
  KDTreeMatcher:
    knn: 1
    maxDist: 10.0
outlierFilters:
  - MaxDistOutlierFilter:
      maxDist: 3.0
  - NullOutlierFilter
  - TrimmedDistOutlierFilter:
      ratio: 0.8
errorMinimizer:
  PointToPointErrorMinimizer
transformationCheckers:
  - CounterTransformationChecker:
      maxIterationCount: 40
  - DifferentialTransformationChecker:
      minDiffRotErr: 0.01
      minDiffTransErr: 0.1
      smoothLength: 4
inspector:
  NullInspector
logger:
  NullLogger
"""


@pytest.mark.parametrize("minimizer", [0, 2])
def test_module_equivalences(ctx, minimizer):
    srcs, tgts, jobs4, g, _ = _pools(51)
    S, T = np.concatenate(srcs), np.concatenate(tgts)
    p = icp_config.shipped_params(minimizer=minimizer)
    plain = _jobs(ctx, p, S, T, jobs4, g)
    assert (plain[0] == 0).all()
    _same(_jobs(ctx, K.chain3(p), S, T, jobs4, g), plain)                                   # nothing listed
    _same(_jobs(ctx, K.chain3(p, use_min_dist=1, min_dist=0.0), S, T, jobs4, g), plain)     # MinDist {0}
    if minimizer == 0:                                                                      # NullOutlierFilter, parsed
        null = icp_config.parse_icp_chain(SHIPPED_WITH_NULL, dims=3)
        assert null.dims == 3 and not null.has_modules() and null.params.as_dict() == p.as_dict()
        _same(_jobs(ctx, null, S, T, jobs4, g), plain)
    far = dict(use_bound=1, max_rotation_norm=3.0, max_translation_norm=50.0)
    for order in range(4):
        _same(_jobs(ctx, K.chain3(p, bound_order=order, **far), S, T, jobs4, g), plain)      # an unreachable Bound
    # MedianDist {1} is TrimmedDist {0.5}: the same order statistic as the limit
    p_half = icp_config.shipped_params(minimizer=minimizer, trim_ratio=0.5)
    p_none = icp_config.shipped_params(minimizer=minimizer, use_trimmed_filter=0)
    _same(_jobs(ctx, K.chain3(p_none, use_median=1, median_factor=1.0), S, T, jobs4, g), _jobs(ctx, p_half, S, T, jobs4, g))
    # the C call with NULL outliers and no stages, and with an all-zero structure
    st, Tm, it = np.zeros(len(g), np.int32), np.zeros((len(g), 4, 4), f32), np.zeros(len(g), np.int32)
    for ox in (None, C.byref(L.IcpOutliers())):
        with ctx.lock:
            ctx._check(ctx.lib.sfe_icp3_compute_jobs_chain_ext(
                ctx.handle, C.byref(p), ox, None, 0, None, 0, L.ptr(S, C.c_float), len(S), L.ptr(T, C.c_float), len(T),
                L.ptr(jobs4, C.c_int32), L.ptr(g, C.c_float), len(g), L.ptr(Tm, C.c_float), L.ptr(st, C.c_int32),
                L.ptr(it, C.c_int32)))
        _same((st, Tm, it), plain)


@pytest.mark.parametrize("minimizer", [0, 2])
def test_store_route_is_compute_jobs_with_the_same_chain(ctx, minimizer):
    srcs, tgts, jobs4, g, pick = _pools(61)
    chain = K.chain3(icp_config.shipped_params(minimizer=minimizer), [D.max_dist(3.3)], [D.octree(0.15), D.min_dist(0.1)],
                     use_median=1, median_factor=2.5, use_min_dist=1, min_dist=0.002, use_bound=1, max_rotation_norm=1.0,
                     max_translation_norm=5.0, bound_order=3)
    want = _jobs(ctx, chain, np.concatenate(srcs), np.concatenate(tgts), jobs4, g)
    s = store.CloudStore3(ctx, capacity_points=1 << 14, max_clouds=16)
    hs, ht = [s.put(c) for c in srcs], [s.put(c) for c in tgts]
    before = (len(s), s.meta())
    got = s.icp([[hs[i], ht[j]] for i, j, _ in pick], g, chain)
    _same(got, want)
    assert (got[0] == 0).all()
    after = (len(s), s.meta())
    assert before[0] == after[0] and all(np.array_equal(a, b) for a, b in zip(before[1], after[1]))
    for h, c in zip(hs + ht, srcs + tgts):
        assert np.array_equal(s.read(h), c)


# ---- against the reference ---------------------------------------------------------------------------------------------------
def _hold(ctx, src, tgt, g, chain, info, normals_of=None):
    """one job through compute_jobs against icp3_chain_ref on the clouds the reference filters itself"""
    st, T, it = _jobs(ctx, chain, src, tgt, [[0, len(src), 0, len(tgt)]], g)
    fs, ft = D.apply(src, chain.reading, _ds(ctx)), D.apply(tgt, chain.reference, _ds(ctx))
    if len(fs) == 0 or len(ft) == 0:
        want = (7, np.asarray(g, f32), 0)
    else:
        want = R.icp(fs, ft, g, chain.params, chain.outliers if chain.outliers.any() else None, normals_of=normals_of)
    d = _diff(T[0], want[1]) if want[0] == 0 else None
    print(info, "status", int(st[0]), want[0], "iterations", int(it[0]), want[2], "diff", d)
    assert (int(st[0]), int(it[0])) == (want[0], want[2]), info
    if want[0] == 0:
        assert d < TOL_TIGHT, (info, d)
    else:
        assert np.array_equal(T[0], np.asarray(g, f32)), info
    return int(st[0]), T[0], int(it[0])


MODULES = dict(use_median=1, median_factor=2.0, use_min_dist=1, min_dist=0.003, use_bound=1, max_rotation_norm=1.0,
               max_translation_norm=5.0, bound_order=1)


@pytest.mark.parametrize("ns", [1, 1024, 1025, 2048, 2049, 2500])
def test_source_counts_at_the_lane_ownership_edges(ctx, ns):
    src, tgt, g = K.pair(100 + ns, ns, 700)
    st, _, it = _hold(ctx, src, tgt, g, K.chain3(icp_config.shipped_params(max_iter=6), **MODULES), "ns%d" % ns)
    assert st == 0 or ns == 1


@pytest.mark.parametrize("nt", [4096, 4097])
def test_target_counts_at_the_tile_edge(ctx, nt):
    src, tgt, g = K.pair(200 + nt, 600, nt)
    assert _hold(ctx, src, tgt, g, K.chain3(icp_config.shipped_params(max_iter=5), **MODULES), "nt%d" % nt)[0] == 0


def test_a_streamed_target_filtered_to_a_resident_one(ctx):
    src, tgt, g = K.pair(301, 500, 4300)
    rf = [D.max_dist(2.5, 0)]
    kept = len(D.apply(tgt, rf))
    assert 3000 < kept <= 4096 < len(tgt)
    chain = K.chain3(icp_config.shipped_params(max_iter=5), reference=rf, **MODULES)
    assert _hold(ctx, src, tgt, g, chain, "4300 -> %d" % kept)[0] == 0


@pytest.mark.parametrize("minimizer", [0, 2])
def test_a_target_filtered_to_one_point(ctx, minimizer):
    src, tgt, g = K.pair(302, 200, 400)
    tgt[7] = (20.0, 0.5, 0.5)
    chain = K.chain3(icp_config.shipped_params(minimizer=minimizer, matcher_max_dist=100.0, use_max_dist_filter=0),
                     reference=[D.min_dist(10.0, 0)], use_median=1, median_factor=3.0)
    assert len(D.apply(tgt, chain.reference)) == 1
    st, _, _ = _hold(ctx, src, tgt, g, chain, "one target point, minimizer %d" % minimizer)
    assert st == (5 if minimizer == 2 else 0)


@pytest.mark.parametrize("name", ["min_dist", "median"])
def test_pairs_exactly_on_a_threshold_and_one_ulp_either_side(ctx, name):
    # (tests/test_icp3_chain_host.py: the distances are exact, and '>' for '>=' or a median over all d2 moves the pose by
    # more than 1000 x the bar)
    tgt, (src, grp) = K.lattice_target(), K.lattice_source()
    ox = K.MIN_DIST_ON if name == "min_dist" else K.MEDIAN_ON
    st, T, it = _hold(ctx, src, tgt, np.eye(4, dtype=f32), K.chain3(K.lattice_params(), **ox), "lattice " + name)
    assert (st, it) == (0, 1)
    for wrong in ("min_strict", "median_all"):
        if wrong.startswith(name[:3]):
            bad = R.icp(src, tgt, np.eye(4, dtype=f32), K.lattice_params(), L.IcpOutliers(**ox), wrong=wrong)
            assert _diff(T, bad[1]) > 1000 * TOL_TIGHT


def test_failure_statuses_beside_healthy_jobs_in_one_launch(ctx):
    src, tgt, g = K.pair(303, 400, 500)
    far = K.far_source(80)
    S = np.concatenate([src, far])
    jobs4 = [[0, len(src), 0, len(tgt)], [len(src), len(far), 0, len(tgt)], [0, len(src), 0, len(tgt)]]
    gs = np.stack([g, g, C3.GUESS.astype(f32)])
    # no finite distance under MedianDist: "no outlier to filter"
    p = icp_config.shipped_params(use_trimmed_filter=0)
    chain = K.chain3(p, use_median=1, median_factor=3.0)
    st, T, it = _jobs(ctx, chain, S, tgt, jobs4, gs)
    assert st.tolist() == [0, 1, 0] and it[1] == 0 and np.array_equal(T[1], g)
    for k in (0, 2):
        want = R.icp(src, tgt, gs[k], p, chain.outliers)
        assert (want[0], want[2]) == (0, int(it[k])) and _diff(T[k], want[1]) < TOL_TIGHT
    # a job emptied by its reading filter: status 7, T = the guess, beside the healthy ones
    chain = K.chain3(p, reading=[D.max_dist(50.0)], use_median=1, median_factor=3.0)
    st7, T7, it7 = _jobs(ctx, chain, S, tgt, jobs4, gs)
    assert st7.tolist() == [0, 7, 0] and it7[1] == 0 and np.array_equal(T7[1], g)
    assert np.array_equal(T7[0], T[0]) and np.array_equal(T7[2], T[2]) and np.array_equal(it7[[0, 2]], it[[0, 2]])
    # ... and by its reference filter, every job of the launch
    chain = K.chain3(p, reference=[D.min_dist(500.0)])
    st7, T7, it7 = _jobs(ctx, chain, S, tgt, jobs4, gs)
    assert st7.tolist() == [7, 7, 7] and not it7.any() and np.array_equal(T7, gs)


@pytest.mark.parametrize("minimizer", [0, 2])
def test_bound_by_rotation_and_by_translation(ctx, minimizer):
    src, tgt, g = K.pair(304, 500, 600)
    p = icp_config.shipped_params(minimizer=minimizer)
    for lim in (dict(max_rotation_norm=0.01, max_translation_norm=5.0), dict(max_rotation_norm=1.0, max_translation_norm=0.02)):
        st, T, it = _hold(ctx, src, tgt, g, K.chain3(p, use_bound=1, bound_order=0, **lim), "bound %r" % (lim,))
        assert st == 9 and it >= 1 and np.array_equal(T, g)
        assert pcl.ICP(ctx) is not None and L.ICP_STATUS_MESSAGES[9] == "limit out of bounds"


@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_bound_listed_before_and_after_counter_and_differential(ctx, order):
    src, tgt, g = K.pair(305, 500, 600)
    tight = dict(use_bound=1, max_rotation_norm=1e-4, max_translation_norm=1e-4, bound_order=order)
    # the Counter ends the job at the iteration at which Bound would stop it: behind the Counter Bound is never asked
    st, _, it = _hold(ctx, src, tgt, g, K.chain3(icp_config.shipped_params(max_iter=1), **tight), "bound order %d, 1 iteration" % order)
    assert (st, it) == ((0, 1) if order & 1 else (9, 1))
    # with iterations to spare it stops the job wherever it is listed
    loose = dict(tight, max_rotation_norm=0.02, max_translation_norm=0.05)
    st, _, it = _hold(ctx, src, tgt, g, K.chain3(icp_config.shipped_params(), **loose), "bound order %d" % order)
    assert st == 9


def test_planar_clouds_give_the_2d_chains_result(ctx):
    src, tgt, g4 = C3.planar_pair(306, 900, 1000)
    ox = dict(use_median=1, median_factor=2.0, use_min_dist=1, min_dist=0.003, use_bound=1, max_rotation_norm=1.0,
              max_translation_norm=5.0, bound_order=3)
    rd, rf = [D.max_dist(3.5), D.min_dist(0.05, 1)], [D.box((-2.9, -2.9, -1.0), (2.9, 2.9, 1.0), 0), D.max_dist(2.5, 0)]
    p = icp_config.shipped_params()
    icp3 = pcl.ICP(ctx)
    icp3.setChain(K.chain3(p, rd, rf, **ox))
    m3, T3, it3 = icp3.compute_batch(src, tgt, [g4])
    rf2 = [D.stage(L.DPF_BOUNDING_BOX, -1, 0, (-2.9, 2.9, -2.9, 2.9, -1.0, 1.0)), D.max_dist(2.5, 0)]
    icp2 = pcl.ICP(ctx)
    icp2.setChain(icp_config.IcpChain(p, rd, rf2, L.IcpOutliers(**ox)))
    m2, T2, it2 = icp2.compute_batch(src[:, :2].copy(), tgt[:, :2].copy(), [C3.guess3(g4)])
    print("planar chain: 3-D against 2-D", m3, m2, it3, it2, _diff(T3[0], icp3_ref.embed(T2[0])))
    assert m3 == m2 == ["success"] and it3[0] == it2[0]
    assert _diff(T3[0], icp3_ref.embed(T2[0])) < TOL_TIGHT


@pytest.mark.parametrize("minimizer", [0, 2])
def test_thirty_guesses_filter_each_cloud_once(ctx, minimizer):
    src, tgt, _ = K.pair(307, 800, 900)
    guesses = C3.batch_guesses(30)
    p = icp_config.shipped_params(minimizer=minimizer)
    rd, rf = [D.min_dist(0.1)], [D.octree(0.2)]
    chain = K.chain3(p, rd, rf, use_median=1, median_factor=2.5)
    icp = pcl.ICP(ctx)
    icp.setChain(chain)
    m, T, it = icp.compute_batch(src, tgt, guesses)                     # the clouds identified by id: one slice each
    # the clouds identified by slice: 30 jobs on the same two slices, behind a cloud nobody uses
    pad = np.full((17, 3), 9.0, f32)
    jobs4 = np.tile(np.array([[17, len(src), 17, len(tgt)]], np.int32), (30, 1))
    st, T2, it2 = icp.compute_jobs(np.concatenate([pad, src]), np.concatenate([pad, tgt]), jobs4,
                                   np.stack(guesses).astype(f32).reshape(30, 16))
    assert np.array_equal(T.view(np.uint32), T2.view(np.uint32)) and np.array_equal(it, it2) and not st.any()
    assert m == ["success"] * 30
    # ICP on the clouds filtered beforehand: with minimizer 2 the normals are those of the filtered target
    fs, ft = D.apply(src, rd), pcl.downsample(tgt, 0.2, ctx=ctx)
    pre = pcl.ICP(ctx)
    pre.setChain(K.chain3(p, use_median=1, median_factor=2.5))
    _, T3, it3 = pre.compute_batch(fs, ft, guesses)
    assert np.array_equal(T.view(np.uint32), T3.view(np.uint32)) and np.array_equal(it, it3)
    if minimizer == 2:
        mean = np.array([f32(np.cumsum(ft[:, a].astype(np.float64))[-1] / len(ft)) for a in range(3)], f32)
        nv = pcl.surface_normals(ft - mean, p.normals_knn, ctx=ctx)
        for k in (0, 29):
            want = R.icp(fs, ft, guesses[k], p, chain.outliers, normals_of=nv)
            assert (want[0], want[2]) == (0, int(it[k])) and _diff(T[k], want[1]) < TOL_TIGHT
