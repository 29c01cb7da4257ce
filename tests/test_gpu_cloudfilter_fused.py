"""GPU: the resident cloud filters with the outlier filter in the downsample kernel's tail (sfe_cloudfilter.hip).

Every case goes through sfe_cloud_filter_batch_dev (the store's and the chain filter's own calls once each through their
public entry points) and is compared bit for bit, clouds and counts, with what FeatureExtraction.callback computes
(feature_extraction.py:241-249): oracle.downsample where the resolution is > 0, then oracle.remove_outlier where
min_points is > 1.  Frames are built on the octree the filter builds: two anchor points fix the bounding box, so that
at 0.5 m a leaf is one cell of a 0.5 m grid and a case can say how many leaves there are and how long each one is.

Leaf lengths: the per-leaf work of the downsample kernel is one lane per leaf; 8 / 16 / 32 are the lengths at which a
split between short and long leaves would sit, 64 / 65 one wave's width, 300 several trips of a wave; 1023 .. 2100
leaves are one, just over one and more than two rounds of the 1024 lanes.  Routes: the frames the tail cannot take
(sorted by another launch, no cell level for the radius, more than 8192 leaves) reach cf_radius_filter_kernel through a
list; they are tested alone, mixed into one call, and in a call of more frames than the device has CUs."""
import ctypes as C

import numpy as np
import pytest

import oracle
from sonar_slam_amd import _lib as L
from sonar_slam_amd import icp_config
from sonar_slam_amd import store as st

from dpf_ref import stage

pytestmark = pytest.mark.gpu

RES, RAD, MINP = 0.5, 1.0, 5     # feature.yaml's filters
SIDE = 64.0                      # anchored frames: a 64 m box -> 7 levels, 128 x 128 leaves of 0.5 m


def expected(pts, res, rad, minp):
    p = np.ascontiguousarray(pts, np.float64).reshape(-1, 2).astype(np.float32)
    if res > 0 and len(p):
        p = oracle.downsample(p, res)
    if minp > 1 and len(p):
        p = oracle.remove_outlier(p, rad, minp)
    return p


def run(ctx, frames, cap, res=RES, rad=RAD, minp=MINP):
    """sfe_cloud_filter_batch_dev on the frames (float64 [n][cap][2] + counts) -> (counts, list of clouds)"""
    n = len(frames)
    pts = np.full((n, cap, 2), 1e30, np.float64)
    cnt = np.zeros(n, np.int32)
    for f, p in enumerate(frames):
        p = np.asarray(p, np.float64).reshape(-1, 2)
        assert len(p) <= cap
        pts[f, :len(p)] = p
        cnt[f] = len(p)
    d_pts, d_cnt, d_out, d_ocnt = ctx.alloc(pts.nbytes), ctx.alloc(4 * n), ctx.alloc(n * cap * 8), ctx.alloc(4 * n)
    try:
        d_pts.upload(pts)
        d_cnt.upload(cnt)
        d_out.zero()
        d_ocnt.upload(np.full(n, -77, np.int32))
        ctx._check(ctx.lib.sfe_cloud_filter_batch_dev(ctx.handle, d_pts.ptr, d_cnt.ptr, n, cap, res, rad, minp, d_out.ptr, d_ocnt.ptr))
        ctx.sync()
        ocnt = d_ocnt.download(np.int32, n)
        out = d_out.download(np.float32, n * cap * 2).reshape(n, cap, 2)
    finally:
        for b in (d_pts, d_cnt, d_out, d_ocnt):
            b.free()
    return ocnt, [out[f, :max(int(ocnt[f]), 0)] for f in range(n)]


def check(ctx, frames, cap, res=RES, rad=RAD, minp=MINP, want=None, what=""):
    ocnt, clouds = run(ctx, frames, cap, res, rad, minp)
    want = want if want is not None else [expected(p, res, rad, minp) for p in frames]
    for f, (w, c) in enumerate(zip(want, clouds)):
        if w is None:                       # tree deeper than 24 levels: refused
            assert ocnt[f] == -1, (what, f, ocnt[f])
            continue
        assert ocnt[f] == len(w), "%s frame %d (%d points): %d in the cloud, the oracle has %d" % (what, f, len(frames[f]), ocnt[f], len(w))
        assert np.array_equal(c.view(np.uint32), w.view(np.uint32)), "%s frame %d: another cloud than the oracle's" % (what, f)
    return ocnt, want


ANCHORS = np.array([[0.0, 0.0], [SIDE, SIDE]])


def leaves_frame(rng, sizes, cells=None, clustered=True, anchors=True):
    """one frame with a leaf of sizes[k] points in the k-th chosen cell of the 128 x 128 grid (never an anchor's cell);
    clustered: the cells form a blob around the middle, so that the outlier filter keeps some points and removes others;
    the points are shuffled, so that the sort has something to do"""
    if cells is None:
        ij = np.array([(i, j) for i in range(2, 126) for j in range(2, 126)])
        if clustered:
            d = np.hypot(ij[:, 0] - 64, ij[:, 1] - 64) + rng.uniform(0, 25, len(ij))
            ij = ij[np.argsort(d, kind="stable")]
            cells = ij[:len(sizes)]
        else:
            cells = ij[rng.permutation(len(ij))[:len(sizes)]]
    pts = [ANCHORS] if anchors else []
    for (i, j), k in zip(cells, sizes):
        pts.append(np.c_[rng.uniform(0.5 * i + 0.03, 0.5 * i + 0.47, k), rng.uniform(0.5 * j + 0.03, 0.5 * j + 0.47, k)])
    p = np.concatenate(pts)
    return p[rng.permutation(len(p))]


def n_leaves(p):
    return len(oracle.downsample(np.asarray(p, np.float32), RES))


# ---- leaf shapes ------------------------------------------------------------------------------------------------------
def test_tiny_frames_one_leaf_and_a_leaf_per_point(ctx):
    rng = np.random.default_rng(1)
    one_leaf = np.c_[rng.uniform(3.0, 3.2, 500), rng.uniform(-7.2, -7.0, 500)]        # a 0.2 m box: no level at all
    grid = np.array([(0.5 * i + 0.25, 0.5 * j + 0.25) for i in range(40, 80) for j in range(40, 80)])   # 1600 leaves of one
    per_point = np.concatenate([ANCHORS, grid + rng.uniform(-0.2, 0.2, grid.shape)])
    frames = [np.zeros((0, 2)), np.array([[1.0, 2.0]]), np.array([[1.0, 2.0], [9.0, -4.0]]), np.array([[1.0, 2.0], [1.1, 2.1]]),
              one_leaf, per_point[rng.permutation(len(per_point))]]
    ocnt, want = check(ctx, frames, 2048, what="tiny")
    assert n_leaves(one_leaf) == 1 and n_leaves(per_point) == 1602
    assert 0 < ocnt[5] < 1602           # the filter removed the anchors and kept the grid
    check(ctx, frames, 2048, minp=1, what="tiny, copy")


LEAF_LENGTHS = [8, 9, 16, 17, 32, 33, 64, 65, 300]


@pytest.mark.parametrize("k", LEAF_LENGTHS)
def test_leaves_of_one_length(ctx, k):
    rng = np.random.default_rng(100 + k)
    p = leaves_frame(rng, [k] * 40)
    assert n_leaves(p) == 42
    check(ctx, [p], 16384, what="leaves of %d" % k)


def test_mixed_leaf_lengths_in_one_frame(ctx):
    rng = np.random.default_rng(2)
    sizes = LEAF_LENGTHS * 3 + [1] * 700 + [2] * 300 + [3, 5, 7, 20, 39, 94, 125] * 4
    p = leaves_frame(rng, [sizes[i] for i in rng.permutation(len(sizes))])
    ocnt, want = check(ctx, [p, p[::-1].copy()], 16384, what="mixed")
    assert n_leaves(p) == len(sizes) + 2 and 0 < ocnt[0] < len(sizes) + 2
    check(ctx, [p], 32768, what="mixed, capacity 32768")


@pytest.mark.parametrize("leaves", [1023, 1024, 1025, 2100])
def test_leaf_counts_around_the_round_of_1024(ctx, leaves):
    rng = np.random.default_rng(leaves)
    sizes = rng.choice([1, 1, 1, 2, 2, 3, 6, 12], leaves - 2)
    p = leaves_frame(rng, sizes)
    assert n_leaves(p) == leaves
    ocnt, _ = check(ctx, [p], 8192, what="%d leaves" % leaves)
    assert 0 < ocnt[0] < leaves


# ---- ties -------------------------------------------------------------------------------------------------------------
def _medoid_distances(leaf):
    """the kernel's float32 recipe: centroid = chain of additions in index order / count, distance = sqrt(dx^2 + dy^2)"""
    s = np.zeros(2, np.float32)
    for q in leaf.astype(np.float32):
        s = s + q
    c = s / np.float32(len(leaf))
    d = leaf.astype(np.float32) - c
    return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])


def test_ties_inside_a_leaf(ctx):
    rng = np.random.default_rng(3)
    leaves = []
    # duplicated points; two points at the same distance from an exactly representable centroid, both orders: the lower index wins
    leaves.append(np.repeat(np.array([[5.125, 5.25], [5.375, 5.25]]), 3, axis=0))
    leaves.append(np.array([[8.125, 5.25], [8.375, 5.25]]))
    leaves.append(np.array([[11.375, 5.25], [11.125, 5.25]]))
    leaves.append(np.array([[14.25, 5.125], [14.25, 5.375], [14.125, 5.25], [14.375, 5.25]]))
    # leaves whose smallest distances differ by one ulp, found by search with the kernel's float32 recipe: points on
    # nearly the same circle around the cell's middle -- three of them (a, b, -(a + b)), or two symmetric pairs, where each
    # pair ties exactly and the pairs are one ulp apart
    one_ulp = []
    for _ in range(20000):
        c = np.array([1.25 + 1.5 * len(one_ulp), 1.25], np.float32)
        r, t1, t2 = rng.uniform(0.08, 0.2), rng.uniform(0, np.pi), rng.uniform(0, np.pi)
        a, b = np.float32(r) * np.array([np.cos(t1), np.sin(t1)], np.float32), np.float32(r) * np.array([np.cos(t2), np.sin(t2)], np.float32)
        pairs = len(one_ulp) % 2 == 1
        leaf = np.array([c + a, c - a, c + b, c - b] if pairs else [c + a, c + b, c - (a + b)], np.float32)
        if np.any(np.abs(leaf - c) > 0.24):
            continue
        d = np.sort(_medoid_distances(leaf))
        lo, hi = (d[1], d[2]) if pairs else (d[0], d[1])
        if lo != hi and np.nextafter(lo, np.float32(100)) == hi and (not pairs or d[0] == d[1]):
            one_ulp.append(leaf.astype(np.float64))
            if len(one_ulp) == 8:
                break
    assert len(one_ulp) == 8
    p = np.concatenate([ANCHORS] + leaves + one_ulp)          # NOT shuffled: the index order is the case
    assert n_leaves(p) == 2 + len(leaves) + len(one_ulp)
    want = oracle.downsample(p.astype(np.float32), RES)
    assert any(np.array_equal(w, [5.125, 5.25]) for w in want) and any(np.array_equal(w, [11.375, 5.25]) for w in want)
    check(ctx, [p], 4096, minp=0, what="ties")
    check(ctx, [p], 4096, rad=4.0, minp=2, what="ties, filtered")


# ---- routes -----------------------------------------------------------------------------------------------------------
def _route_frames():
    rng = np.random.default_rng(4)

    def dense(n):       # n points on the 64 m box: a bench-like frame of ~2000 leaves
        sizes = rng.multinomial(n - 2, np.ones(2000) / 2000)
        return leaves_frame(rng, sizes[sizes > 0])

    deep9 = np.concatenate([np.array([[0.0, 0.0], [200.0, 200.0]]), rng.uniform(60, 90, (3000, 2))])     # 9 levels: the wide sort
    deep25 = np.concatenate([np.array([[-5e6, -5e6], [5e6, 5e6]]), rng.uniform(0, 30, (500, 2))])        # 25 levels: refused
    many = leaves_frame(rng, [1] * 9000 + [2] * 500, clustered=False)                                    # > 8192 leaves: brute force
    narrow = np.c_[rng.uniform(3.0, 3.3, 300), rng.uniform(1.0, 1.3, 300)]                               # root cell < radius: lc < 0
    frames = {"empty": np.zeros((0, 2)), "small": leaves_frame(rng, [3] * 30), "16384": dense(16384), "16385": dense(16385),
              "19456": dense(19456), "19457": dense(19457), "deep9": deep9, "deep25": deep25, "many": many, "narrow": narrow,
              "18945": dense(18945), "typical": dense(11000)}
    want = {k: (None if k == "deep25" else expected(p, RES, RAD, MINP)) for k, p in frames.items()}
    return frames, want


@pytest.fixture(scope="module")
def routes():
    return _route_frames()


def test_routes_one_frame_per_call(ctx, routes):
    frames, want = routes
    assert len(frames["19457"]) == 19457 and len(want["many"]) > 0 and len(oracle.downsample(frames["many"].astype(np.float32), RES)) > 8192
    for k, p in frames.items():
        check(ctx, [p], 32768, want=[want[k]], what=k)


def test_routes_mixed_in_one_call(ctx, routes):
    frames, want = routes
    keys = list(frames)
    assert len(keys) == 12
    check(ctx, [frames[k] for k in keys], 32768, want=[want[k] for k in keys], what="mixed routes")
    keys = keys[::-1]
    check(ctx, [frames[k] for k in keys], 32768, want=[want[k] for k in keys], what="mixed routes, reversed")


def test_more_frames_than_cus(ctx, routes):
    frames, want = routes
    rng = np.random.default_rng(5)
    pool = [k for k in frames if len(frames[k]) <= 4096] + ["thin"]
    frames = dict(frames, thin=leaves_frame(rng, rng.choice([1, 2, 5, 30], 350)))
    want = dict(want, thin=expected(frames["thin"], RES, RAD, MINP))
    deal = [pool[i] for i in rng.integers(0, len(pool), 257)]
    assert {"empty", "small", "deep9", "deep25", "narrow", "thin"} <= set(deal)
    check(ctx, [frames[k] for k in deal], 4096, want=[want[k] for k in deal], what="257 frames")


def test_radius_wider_than_the_root_cell(ctx, routes):
    frames, _ = routes
    keys = ["empty", "small", "typical", "narrow"]
    check(ctx, [frames[k] for k in keys], 16384, rad=100.0, minp=40, what="radius 100")


# ---- modes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [8192, 16384, 32768])
@pytest.mark.parametrize("res,rad,minp", [(RES, RAD, 0), (RES, RAD, 1), (0.0, RAD, MINP), (-1.0, RAD, 0), (RES, 0.0, 2), (RES, 0.0, 0),
                                          (RES, RAD, MINP), (0.25, 0.6, 3)])
def test_modes_and_capacities(ctx, routes, cap, res, rad, minp):
    rng = np.random.default_rng(cap)
    frames, _ = routes
    dup = np.repeat(leaves_frame(rng, [1] * 200), 3, axis=0)                   # every point three times: radius 0 keeps them at min_points 2
    fr = [frames["empty"], frames["small"], dup, leaves_frame(rng, rng.choice([1, 2, 4, 12], 1500)), frames["narrow"]]
    if res <= 0:
        fr = [p[:3000] for p in fr]      # (the radius filter alone is brute force)
    ocnt, want = check(ctx, fr, cap, res, rad, minp, what=(cap, res, rad, minp))
    if res > 0 and rad == 0.0 and minp == 2:
        assert ocnt[2] == 0 and ocnt[3] == 0       # the downsample left no duplicates


def test_the_store_and_the_chain_filter_call(ctx):
    """their own sfe_cf_run_staged calls (radius 0, min_points 0: the plain copy), through the public entry points"""
    rng = np.random.default_rng(6)
    clouds = [leaves_frame(rng, rng.choice([1, 2, 4, 25, 70], 1200)).astype(np.float32), np.zeros((0, 2), np.float32),
              leaves_frame(rng, [3] * 50).astype(np.float32)]
    s = st.CloudStore(ctx, capacity_points=1 << 17, max_clouds=32)
    hs = [s.put(c) for c in clouds]
    eye = st.pose_T6(np.eye(3))
    out = s.get_points(np.array([[hs[0], -1], [hs[1], -1], [hs[2], hs[0]]], np.int32), np.array([[eye, eye]] * 3, np.float32), RES,
                       flags=st.F32_POINTS)
    for h, src in zip(out, (clouds[0], clouds[1], np.concatenate([clouds[2], clouds[0]]))):
        want = oracle.downsample(src, RES) if len(src) else src
        assert np.array_equal(s.read(h), want)
    s.close()

    arr, n = icp_config.IcpChain.device_stages([stage(L.DPF_OCTREE_GRID, f=[RES])])
    off = np.zeros(len(clouds) + 1, np.int32)
    off[1:] = np.cumsum([len(c) for c in clouds])
    flat = np.concatenate(clouds)
    d_in, d_out = ctx.alloc(flat.nbytes), ctx.alloc(flat.nbytes)
    counts = np.zeros(len(clouds), np.int32)
    try:
        d_in.upload(flat)
        with ctx.lock:
            ctx._check(ctx.lib.sfe_icp_filter_clouds_dev(ctx.handle, arr, n, d_in.ptr, L.ptr(off, C.c_int32), len(clouds), d_out.ptr,
                                                         L.ptr(counts, C.c_int32)))
            got = d_out.download(np.float32, 2 * int(counts.sum())).reshape(-1, 2)
    finally:
        d_in.free()
        d_out.free()
    want = [oracle.downsample(c, RES) if len(c) else c for c in clouds]
    assert counts.tolist() == [len(w) for w in want] and np.array_equal(got, np.concatenate(want))
