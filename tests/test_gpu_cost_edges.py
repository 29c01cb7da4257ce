"""The matching-cost kernels (csrc/sfe_cost.hip) where they change behaviour: the row / column clipping and the word masks of the
stamp kernels, the clamp of the stamp-points kernel, the cell arithmetic of both scoring kernels in both dtypes (near-ties of the
float64 multiplication short cut, true ties, grid edges, non-finite points, the float32 fused multiply-add), the wave and
workgroup tails over source and pose counts, the LDS limit and the L2 route.  The C entry points are called the way
matching_cost.py calls them, with rows / cols / hs / origin as the case needs them.  Every expectation is exact and comes from
tests/cost_ref.py; tests/test_cost_ref_host.py checks that reference and the constructed cases on the CPU."""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cost_ref as R  # noqa: E402
from sonar_slam_amd import _lib as L  # noqa: E402
from sonar_slam_amd import store as st  # noqa: E402
from sonar_slam_amd.chained import Pose2Batch, sample_transforms  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
F64_POINTS = 1      # SFE_COST_F64_POINTS
DTYPES = pytest.mark.parametrize("f64", [True, False], ids=["f64_points", "f32_points"])
MANY = 35           # poses of a padded set: the many-pose kernel (>= 32), a wave with three poses at the end


# ---- the C entry points -------------------------------------------------------------------------------------------------------
def create(ctx, r, c, rows, cols, hs):
    r, c = np.ascontiguousarray(r, np.int32), np.ascontiguousarray(c, np.int32)
    h = C.c_void_p()
    with ctx.lock:
        ctx._check(ctx.lib.sfe_costgrid_create(ctx.handle, L.ptr(r, C.c_int32), L.ptr(c, C.c_int32), len(r), int(rows), int(cols),
                                               int(hs), C.byref(h)))
    return h


def create_store(ctx, store, handles, xmin, ymin, res, rows, cols, hs):
    th = np.ascontiguousarray(handles, np.int32).reshape(-1)
    x0, y0 = np.ascontiguousarray(xmin, F32).reshape(-1), np.ascontiguousarray(ymin, F32).reshape(-1)
    rows, cols = np.ascontiguousarray(rows, np.int32).reshape(-1), np.ascontiguousarray(cols, np.int32).reshape(-1)
    assert len(th) == len(x0) == len(y0) == len(rows) == len(cols)
    h = C.c_void_p()
    with ctx.lock:
        ctx._check(ctx.lib.sfe_costgrid_create_store(ctx.handle, store.handle, L.ptr(th, C.c_int32), len(th), L.ptr(x0, C.c_float),
                                                     L.ptr(y0, C.c_float), F32(res), L.ptr(rows, C.c_int32), L.ptr(cols, C.c_int32),
                                                     int(hs), C.byref(h)))
    return h


def destroy(ctx, h):
    if h is not None and h.value:
        ctx.lib.sfe_costgrid_destroy(h)


def download(ctx, h, index, rows, cols):
    out = np.full((int(rows), int(cols)), 7, np.uint8)
    with ctx.lock:
        ctx._check(ctx.lib.sfe_costgrid_download(ctx.handle, h, int(index), L.ptr(out, C.c_uint8)))
    return out


def score_batch(ctx, h, src, T6, xmin, ymin, res, f64):
    src = np.ascontiguousarray(src, F32).reshape(-1, 2)
    T6 = np.ascontiguousarray(T6, F32).reshape(-1, 6)
    out = np.full(len(T6), 12345, np.int32)
    with ctx.lock:
        ctx._check(ctx.lib.sfe_matching_cost_batch(ctx.handle, h, L.ptr(src, C.c_float), len(src), L.ptr(T6, C.c_float), len(T6),
                                                   F32(xmin), F32(ymin), float(res), F64_POINTS if f64 else 0, L.ptr(out, C.c_int32)))
    return out


def score_store(ctx, h, store, source_handles, grid_index, T6, res, f64):
    sh = np.ascontiguousarray(source_handles, np.int32).reshape(-1)
    gi = None if grid_index is None else np.ascontiguousarray(grid_index, np.int32).reshape(-1)
    T6 = np.ascontiguousarray(T6, F32).reshape(len(sh), -1, 6)
    out = np.full((len(sh), T6.shape[1]), 12345, np.int32)
    with ctx.lock:
        ctx._check(ctx.lib.sfe_matching_cost_store(ctx.handle, h, store.handle, L.ptr(sh, C.c_int32),
                                                   None if gi is None else L.ptr(gi, C.c_int32), len(sh), L.ptr(T6, C.c_float),
                                                   T6.shape[1], float(res), F64_POINTS if f64 else 0, L.ptr(out, C.c_int32)))
    return out


def score_samples(ctx, h, store, source_handles, grid_index, target4, source4, delta4, res, f64):
    sh = np.ascontiguousarray(source_handles, np.int32).reshape(-1)
    gi = None if grid_index is None else np.ascontiguousarray(grid_index, np.int32).reshape(-1)
    t4 = np.ascontiguousarray(target4, np.float64).reshape(len(sh), 4)
    s4 = np.ascontiguousarray(source4, np.float64).reshape(len(sh), 4)
    d4 = np.ascontiguousarray(delta4, np.float64).reshape(-1, 4)
    out = np.full((len(sh), len(d4)), 12345, np.int32)
    with ctx.lock:
        ctx._check(ctx.lib.sfe_matching_cost_store_samples(ctx.handle, h, store.handle, L.ptr(sh, C.c_int32),
                                                           None if gi is None else L.ptr(gi, C.c_int32), len(sh),
                                                           L.ptr(t4, C.c_double), L.ptr(s4, C.c_double), L.ptr(d4, C.c_double), len(d4),
                                                           float(res), F64_POINTS if f64 else 0, L.ptr(out, C.c_int32)))
    return out


def _store(ctx):
    return st.CloudStore(ctx, capacity_points=1 << 16, max_clouds=64)


@functools.lru_cache(maxsize=None)
def _cell_cases():
    return R.cell_cases()


@functools.lru_cache(maxsize=None)
def _want(name, f64):
    """the reference costs of a checkerboard case, computed once"""
    c = _cell_cases()[name]
    w = R.cost(c["grid"], c["src"], c["T6"], c["xmin"], c["ymin"], c["res"], f64)
    w.setflags(write=False)
    return w


# ---- stamp ----------------------------------------------------------------------------------------------------------------------
STAMP_RES, STAMP_XMIN, STAMP_YMIN = 2.0 ** -4, -3.0, 2.0       # dyadic: the cloud on cell centres is exact


@pytest.mark.parametrize("sparse", [False, True], ids=["corners_midpoints_interior", "one_target"])
@pytest.mark.parametrize("shape", R.STAMP_SHAPES, ids=lambda s: "%dx%d_hs%d" % s)
def test_stamp_clips_rows_columns_and_words(ctx, shape, sparse):
    rows, cols, hs = shape
    r, c = R.stamp_case(rows, cols, hs, sparse)
    want = R.grid(r, c, rows, cols, hs)
    h = hs_ = s = None
    try:
        h = create(ctx, r, c, rows, cols, hs)
        assert np.array_equal(download(ctx, h, 0, rows, cols), want)
        # the same targets as a float32 cloud on the cell centres, stamped from the keyframe store
        s = _store(ctx)
        t = s.put(R.centres(r, c, STAMP_XMIN, STAMP_YMIN, STAMP_RES))
        hs_ = create_store(ctx, s, [t], [STAMP_XMIN], [STAMP_YMIN], STAMP_RES, [rows], [cols], hs)
        assert np.array_equal(download(ctx, hs_, 0, rows, cols), want)
    finally:
        destroy(ctx, h)
        destroy(ctx, hs_)
        if s is not None:
            s.close()


@pytest.mark.parametrize("shape", R.OUTSIDE_SHAPES, ids=lambda s: "%dx%d_hs%d" % s)
def test_stamp_of_targets_outside_the_grid_keeps_what_reaches_in(ctx, shape):
    """sfe_costgrid_create takes its targets as given: one outside the grid stamps the part of its element that lies inside"""
    rows, cols, hs = shape
    r, c = R.outside_targets(rows, cols, hs)
    h = None
    try:
        h = create(ctx, r, c, rows, cols, hs)
        assert np.array_equal(download(ctx, h, 0, rows, cols), R.grid(r, c, rows, cols, hs))
    finally:
        destroy(ctx, h)


def test_stamp_without_targets_leaves_the_grid_empty(ctx):
    for rows, cols, hs in ((1, 1, 0), (7, 31, 3), (40, 65, 10)):
        h = None
        try:
            h = create(ctx, np.zeros(0, np.int32), np.zeros(0, np.int32), rows, cols, hs)
            assert np.array_equal(download(ctx, h, 0, rows, cols), np.zeros((rows, cols), np.uint8))
        finally:
            destroy(ctx, h)


# ---- stamp-points ---------------------------------------------------------------------------------------------------------------
def _neighbour(rng, rows, cols, xmin, ymin, res, n):
    pts = np.c_[rng.uniform(xmin, xmin + cols * res, n), rng.uniform(ymin, ymin + rows * res, n)].astype(F32)
    return dict(pts=pts, xmin=F32(xmin), ymin=F32(ymin), rows=rows, cols=cols)


@pytest.mark.parametrize("name", ["clamped", "half_cells", "one_point", "empty", "8193_items"])
def test_stamp_points_between_two_other_grids_of_the_same_object(ctx, name):
    """three grids of different shapes in one object (a non-zero word offset in front of and behind the case's grid): each comes
    back as the reference stamps its own cloud, the neighbours untouched by the case's"""
    case = R.stamp_points_cases()[name]
    rng = np.random.default_rng(121)
    res, hs = case["res"], case["hs"]
    grids = [_neighbour(rng, 7, 37, -5.0, 4.0, res, 3), case, _neighbour(rng, 12, 64, 8.0, -6.0, res, 5)]
    want = [R.stamp_points_grid(dict(g, res=res, hs=hs)) for g in grids]
    assert want[0].any() and want[2].any() and not want[0].all() and not want[2].all()
    s, h = _store(ctx), None
    try:
        handles = [s.put(g["pts"]) for g in grids]
        assert s.counts(handles).tolist() == [3, len(case["pts"]), 5]
        h = create_store(ctx, s, handles, [g["xmin"] for g in grids], [g["ymin"] for g in grids], res, [g["rows"] for g in grids],
                         [g["cols"] for g in grids], hs)
        for k in (1, 0, 2):
            assert np.array_equal(download(ctx, h, k, grids[k]["rows"], grids[k]["cols"]), want[k]), k
    finally:
        destroy(ctx, h)
        s.close()


# ---- cell arithmetic ------------------------------------------------------------------------------------------------------------
CELL_RUNS = [(n, True) for n in ("near_tie_0.03", "near_tie_0.035", "near_tie_0.03_T", "true_tie", "true_tie_T", "edge_of_grid",
                                 "non_finite", "random_checkerboard")] + \
            [(n, False) for n in ("fma", "true_tie", "true_tie_T", "edge_of_grid", "non_finite", "random_checkerboard")]


def _padded(T6, want):
    idx = np.arange(MANY) % len(T6)
    return T6[idx], want[idx]


@pytest.mark.parametrize("name,f64", CELL_RUNS, ids=["%s-%s" % (n, "f64" if f else "f32") for n, f in CELL_RUNS])
def test_cells_on_a_checkerboard_through_both_scoring_kernels(ctx, name, f64):
    c = _cell_cases()[name]
    assert f64 in c["dtypes"]
    want = _want(name, f64)
    T_many, want_many = _padded(c["T6"], want)
    h = None
    try:
        h = create(ctx, c["tgt_r"], c["tgt_c"], c["rows"], c["cols"], 0)
        args = (c["xmin"], c["ymin"], c["res"], f64)
        assert np.array_equal(score_batch(ctx, h, c["src"], T_many, *args), want_many)         # the many-pose kernel
        with ctx.tuning(cost_many=0):
            assert np.array_equal(score_batch(ctx, h, c["src"], T_many, *args), want_many)     # the 8-poses-per-workgroup kernel
        assert np.array_equal(score_batch(ctx, h, c["src"], c["T6"], *args), want)             # ... as the small launch takes it
        assert np.array_equal(download(ctx, h, 0, c["rows"], c["cols"]), c["grid"])
    finally:
        destroy(ctx, h)


STORE_RUNS = [("near_tie_0.03", True), ("near_tie_0.035", True), ("near_tie_0.03_T", True), ("fma", False), ("true_tie", True),
              ("non_finite", False)]


@pytest.mark.parametrize("name,f64", STORE_RUNS, ids=["%s-%s" % (n, "f64" if f else "f32") for n, f in STORE_RUNS])
def test_cells_on_a_checkerboard_over_store_handles(ctx, name, f64):
    """the grid stamped from a cloud on the cell centres, the origin read from the grid's descriptor"""
    c = _cell_cases()[name]
    want = _want(name, f64)
    T_many, want_many = _padded(c["T6"], want)
    s, h = _store(ctx), None
    try:
        t = s.put(R.centres(c["tgt_r"], c["tgt_c"], float(c["xmin"]), float(c["ymin"]), c["res"]))
        q = s.put(c["src"])
        h = create_store(ctx, s, [t], [c["xmin"]], [c["ymin"]], c["res"], [c["rows"]], [c["cols"]], 0)
        assert np.array_equal(download(ctx, h, 0, c["rows"], c["cols"]), c["grid"])
        assert np.array_equal(score_store(ctx, h, s, [q], None, T_many[None], c["res"], f64)[0], want_many)
        with ctx.tuning(cost_many=0):
            assert np.array_equal(score_store(ctx, h, s, [q], None, T_many[None], c["res"], f64)[0], want_many)
        assert np.array_equal(score_store(ctx, h, s, [q], [0], c["T6"][None], c["res"], f64)[0], want)
    finally:
        destroy(ctx, h)
        s.close()


# ---- counts ---------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_source_and_pose_counts_at_wave_and_workgroup_tails(ctx, f64):
    c = R.counts_case()
    args = (c["xmin"], c["ymin"], c["res"], f64)
    h = None
    try:
        h = create(ctx, c["tgt_r"], c["tgt_c"], c["rows"], c["cols"], c["hs"])
        assert np.array_equal(download(ctx, h, 0, c["rows"], c["cols"]), c["grid"])
        for n in R.SOURCE_SIZES:
            want = R.cost(c["grid"], c["src"][:n], c["T6"], *args)
            assert n < 63 or len(set(want.tolist())) >= 5
            for P in R.POSE_COUNTS:
                got = score_batch(ctx, h, c["src"][:n], c["T6"][:P], *args)
                with ctx.tuning(cost_many=0):
                    small = score_batch(ctx, h, c["src"][:n], c["T6"][:P], *args)
                assert np.array_equal(got, want[:P]) and np.array_equal(small, want[:P]), (n, P)
        assert score_batch(ctx, h, c["src"], np.zeros((0, 6), F32), *args).shape == (0,)       # no pose: nothing to do
    finally:
        destroy(ctx, h)


def _xycs(p):
    return np.stack([p.x, p.y, p.c, p.s], axis=1)


@DTYPES
@pytest.mark.parametrize("P", [9, 33], ids=["9_poses", "33_poses"])
def test_store_jobs_of_different_sizes_with_a_repeated_and_a_skipped_grid(ctx, f64, P):
    """three jobs (257, 0 and 65 source points) over the grids 2, 0, 2 of a three-grid object; the same launch with the sample
    transforms computed on the device from the poses"""
    c = R.counts_case()
    rng = np.random.default_rng(131)
    res, hs = c["res"], c["hs"]
    shapes = [(c["rows"], c["cols"], float(c["xmin"]), float(c["ymin"])), (33, 70, 1.0, 1.0), (64, 129, -2.0, -1.5)]
    targets = [(c["tgt_r"], c["tgt_c"])] + [(rng.integers(0, r, 40), rng.integers(0, cc, 40)) for r, cc, _, _ in shapes[1:]]
    want_grids = [R.grid(tr, tc, r, cc, hs) for (tr, tc), (r, cc, _, _) in zip(targets, shapes)]
    sources = [np.c_[rng.uniform(-2.5, 4.5, 257), rng.uniform(-2, 2, 257)].astype(F32), np.zeros((0, 2), F32),
               np.c_[rng.uniform(-2.5, 4.5, 65), rng.uniform(-2, 2, 65)].astype(F32)]
    grid_index = [2, 0, 2]
    tb = Pose2Batch([0.1, -0.2, 0.3], [0.0, 0.1, -0.1], theta=[0.02, -0.03, 0.01])
    sb = Pose2Batch([0.2, 0.0, -0.3], [0.1, -0.1, 0.2], theta=[-0.05, 0.04, 0.08])
    X = np.c_[rng.uniform(-0.5, 0.5, P), rng.uniform(-0.5, 0.5, P), rng.uniform(-0.2, 0.2, P)]
    X[0] = 0
    T6 = sample_transforms(ctx.lib, tb, sb, X)
    assert T6.shape == (3, P, 6)
    d4 = np.stack([X[:, 0], X[:, 1], [math.cos(t) for t in X[:, 2]], [math.sin(t) for t in X[:, 2]]], axis=1)
    want = np.stack([R.cost(want_grids[g], src, T6[j], F32(shapes[g][2]), F32(shapes[g][3]), res, f64)
                     for j, (src, g) in enumerate(zip(sources, grid_index))])
    assert not want[1].any() and len(set(want[0].tolist())) >= 5 and len(set(want[2].tolist())) >= 5
    s, h = _store(ctx), None
    try:
        th = [s.put(R.centres(tr, tc, x0, y0, res)) for (tr, tc), (_, _, x0, y0) in zip(targets, shapes)]
        sh = [s.put(q) for q in sources]
        h = create_store(ctx, s, th, [v[2] for v in shapes], [v[3] for v in shapes], res, [v[0] for v in shapes],
                         [v[1] for v in shapes], hs)
        for k, (r, cc, _, _) in enumerate(shapes):
            assert np.array_equal(download(ctx, h, k, r, cc), want_grids[k]), k
        for many in (1, 0):
            with ctx.tuning(cost_many=many):
                got = score_store(ctx, h, s, sh, grid_index, T6, res, f64)
                sam = score_samples(ctx, h, s, sh, grid_index, _xycs(tb), _xycs(sb), d4, res, f64)
            assert np.array_equal(got, want) and np.array_equal(sam, got), many
    finally:
        destroy(ctx, h)
        s.close()


# ---- the LDS limit --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lds_case(name):
    return R.lds_case(*R.LDS_SHAPES[name])


@DTYPES
@pytest.mark.parametrize("name", list(R.LDS_SHAPES))
def test_grids_at_the_lds_limit(ctx, name, f64):
    """768 x 1024 cells are exactly the 24 576 words that fit LDS, 769 x 1024 are read through L2, 768 x 1000 end every row in a
    partial word"""
    c = _lds_case(name)
    args = (c["xmin"], c["ymin"], c["res"], f64)
    want = R.cost(c["grid"], c["src"], c["T6"], *args)
    assert len(want) == 33 and len(set(want[:9].tolist())) >= 5
    h = None
    try:
        h = create(ctx, c["tgt_r"], c["tgt_c"], c["rows"], c["cols"], c["hs"])
        if f64:
            assert np.array_equal(download(ctx, h, 0, c["rows"], c["cols"]), c["grid"])
        for P in (9, 33):
            got = score_batch(ctx, h, c["src"], c["T6"][:P], *args)
            with ctx.tuning(cost_many=0):
                small = score_batch(ctx, h, c["src"], c["T6"][:P], *args)
            assert np.array_equal(got, want[:P]) and np.array_equal(small, want[:P]), P
    finally:
        destroy(ctx, h)


@DTYPES
def test_a_grid_beyond_lds_sends_its_small_neighbour_through_l2_too(ctx, f64):
    big = _lds_case("one_row_more")
    rng = np.random.default_rng(141)
    res, hs = big["res"], big["hs"]
    rows, cols, xmin, ymin = 20, 40, F32(3.0), F32(1.0)
    tr, tc = np.array([10, 0], np.int32), np.array([12, 39], np.int32)
    small_grid = R.grid(tr, tc, rows, cols, hs)
    assert small_grid.any() and not small_grid.all()
    small_src = np.c_[rng.uniform(2.9, 3.0 + cols * res + 0.1, 200), rng.uniform(0.9, 1.0 + rows * res + 0.1, 200)].astype(F32)
    T_small = np.array([R.translation(0, 0)] + [R.rotation(t, x, y) for t, x, y in rng.uniform(-0.2, 0.2, (32, 3))], F32)
    s, h = _store(ctx), None
    try:
        th = [s.put(R.centres(big["tgt_r"], big["tgt_c"], float(big["xmin"]), float(big["ymin"]), res)),
              s.put(R.centres(tr, tc, float(xmin), float(ymin), res))]
        sh = [s.put(big["src"]), s.put(small_src)]
        h = create_store(ctx, s, th, [big["xmin"], xmin], [big["ymin"], ymin], res, [big["rows"], rows], [big["cols"], cols], hs)
        assert np.array_equal(download(ctx, h, 1, rows, cols), small_grid)
        if f64:
            assert np.array_equal(download(ctx, h, 0, big["rows"], big["cols"]), big["grid"])
        for P in (9, 33):
            T6 = np.stack([big["T6"][:P], T_small[:P]])
            want = np.stack([R.cost(big["grid"], big["src"], T6[0], big["xmin"], big["ymin"], res, f64),
                             R.cost(small_grid, small_src, T6[1], xmin, ymin, res, f64)])
            assert len(set(want[1].tolist())) >= 5
            assert np.array_equal(score_store(ctx, h, s, sh, None, T6, res, f64), want), P
            assert np.array_equal(score_store(ctx, h, s, sh[::-1], [1, 0], T6[::-1], res, f64), want[::-1]), P
    finally:
        destroy(ctx, h)
        s.close()
