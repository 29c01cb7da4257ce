"""GPU: the constructed cases of tests/pcl_edges.py through the public ``pcl.*`` calls (and through the C entry points where
the shim refuses: n_ref = 0, sfe_remove_outlier_many), against the C oracle (N x 2) and tests/pcl3_ref.py (N x 3), bit for
bit: ids, d2 as uint32, kept rows, keep masks, densities as uint32, medoids and their indices.  The 3-D calls on z = 0
clouds must equal the 2-D calls.  tests/test_pcl_edges_host.py shows what each case is sensitive to.

One test per kind and width walks its cases and reports every case that differs, so one run shows the whole picture.
"""
import ctypes as C

import numpy as np
import pytest

import pcl_edges as E
from sonar_slam_amd import _lib as L
from sonar_slam_amd import pcl

pytestmark = pytest.mark.gpu
F = np.float32


def dev_match(ctx, ref, pts, knn, m):
    return pcl.match(ref, pts, knn, m, ctx=ctx)


def dev_outlier(ctx, pts, radius, min_points):
    return pcl.remove_outlier(pts, radius, min_points, ctx=ctx)


def dev_density(ctx, pts, knn):
    return pcl.knn_density(pts, knn, ctx=ctx)


def dev_downsample(ctx, pts, res):
    """the descriptor overload: (medoids, their input indices) -- row numbers up to 4097 are exact in float32"""
    out, desc = pcl.downsample(pts, np.arange(len(pts), dtype=F)[:, None], res, ctx=ctx)
    return out, desc[:, 0].astype(np.int32)


def differing(kind, dim, run, want_of):
    return [c.name for c in E.cases(kind, dim) if not E.same(kind, run(c), want_of(c))]


# ---- every case against its reference --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_match_cases(ctx, dim):
    bad = differing("match", dim, lambda c: dev_match(ctx, *c.args), lambda c: E.ref_match(*c.args))
    assert not bad, bad


@pytest.mark.parametrize("dim", [2, 3])
def test_match_random_cases_against_float64(ctx, dim):
    """the device's answer itself (not only the reference's) within the derived rounding bound of the true nearest"""
    n = sum(E.check_against_float64(c, *dev_match(ctx, *c.args)) for c in E.cases("match", dim) if c.name.startswith("sizes_"))
    assert n > 1000


@pytest.mark.parametrize("dim", [2, 3])
def test_remove_outlier_cases(ctx, dim):
    bad = []
    for c in E.cases("outlier", dim):
        rows, _ = E.ref_outlier(*c.args)
        got = dev_outlier(ctx, *c.args)
        if got.shape != rows.shape or got.dtype != F or not np.array_equal(E.bits(got), E.bits(rows)):
            bad.append(c.name)
    assert not bad, bad


@pytest.mark.parametrize("dim", [2, 3])
def test_knn_density_cases(ctx, dim):
    bad = differing("density", dim, lambda c: dev_density(ctx, *c.args), lambda c: E.ref_density(*c.args))
    assert not bad, bad


@pytest.mark.parametrize("dim", [2, 3])
def test_rank_counting_downsample_cases(ctx, dim):
    bad = differing("downsample", dim, lambda c: dev_downsample(ctx, *c.args), lambda c: E.ref_downsample(*c.args))
    assert not bad, bad


@pytest.mark.parametrize("dim", [2, 3])
def test_downsample_without_descriptors_takes_the_same_leaves(ctx, dim):
    """resolution <= 0 keeps the rank-counting route without indices too, and so does every N x 3 call"""
    bad = []
    for c in E.cases("downsample", dim):
        if dim == 3 or not c.args[1] > 0:
            want, _ = E.ref_downsample(*c.args)
            got = pcl.downsample(c.args[0], c.args[1], ctx=ctx)
            if got.shape != want.shape or not np.array_equal(E.bits(got), E.bits(want)):
                bad.append(c.name)
    assert not bad, bad


def test_the_2d_level_cap_on_the_device(ctx):
    """the recorded difference: the device gives the 31-level answer, not the oracle's"""
    out, idx = dev_downsample(ctx, E.LEVEL_CAP_CLOUD, 0.0)
    assert idx.tolist() == E.LEVEL_CAP_KERNEL_IDX and np.array_equal(E.bits(out), E.bits(E.LEVEL_CAP_CLOUD[idx]))


# ---- z = 0: the 3-D kernels on the 2-D cases -------------------------------------------------------------------------------
def test_flat_match_is_the_2d_match(ctx):
    bad = []
    for c in E.cases("match", 2):
        ref, pts, knn, m = c.args
        ids2, d2 = dev_match(ctx, ref, pts, knn, m)
        ids3, d3 = dev_match(ctx, E.z0(ref), E.z0(pts), knn, m)
        if not (np.array_equal(ids3, ids2) and np.array_equal(E.bits(d3), E.bits(d2))):
            bad.append(c.name)
    assert not bad, bad


def test_flat_remove_outlier_is_the_2d_filter(ctx):
    bad = [c.name for c in E.cases("outlier", 2)
           if not np.array_equal(E.bits(dev_outlier(ctx, E.z0(c.args[0]), *c.args[1:])),
                                 E.bits(E.z0(dev_outlier(ctx, *c.args))))]
    assert not bad, bad


def test_flat_knn_density_is_the_2d_density(ctx):
    bad = [c.name for c in E.cases("density", 2)
           if not np.array_equal(E.bits(dev_density(ctx, E.z0(c.args[0]), c.args[1])), E.bits(dev_density(ctx, *c.args)))]
    assert not bad, bad


def test_flat_downsample_is_the_2d_downsample(ctx):
    bad = []
    for c in E.cases("downsample", 2):
        out2, idx2 = dev_downsample(ctx, *c.args)
        out3, idx3 = dev_downsample(ctx, E.z0(c.args[0]), c.args[1])
        if not (np.array_equal(idx3, idx2) and np.array_equal(E.bits(out3), E.bits(E.z0(out2)))):
            bad.append(c.name)
    assert not bad, bad


# ---- through the C entry points --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("knn", [1, 3])
def test_an_empty_reference_cloud_matches_nothing(ctx, dim, knn):
    """n_ref = 0 (pcl.match refuses knn > n_ref like libnabo; the library itself answers -1 / inf for every query)"""
    pts = E.cloud(3, 300, dim)
    ids, d2 = np.full((knn, 300), 7, np.int32), np.full((knn, 300), 7, F)
    sfx = "3" if dim == 3 else ""
    with ctx.lock:
        if knn == 1:
            ctx._check(getattr(ctx.lib, "sfe_match" + sfx)(ctx.handle, None, 0, L.ptr(pts, C.c_float), 300, 1.0,
                                                           L.ptr(ids, C.c_int32), L.ptr(d2, C.c_float)))
        else:
            ctx._check(getattr(ctx.lib, "sfe_match_knn" + sfx)(ctx.handle, None, 0, L.ptr(pts, C.c_float), 300, knn, 1.0,
                                                               L.ptr(ids, C.c_int32), L.ptr(d2, C.c_float)))
    assert (ids == -1).all() and np.isposinf(d2).all()


@pytest.fixture(scope="module")
def many_batches():
    return E.outlier_many_batches()


@pytest.mark.parametrize("k", range(4))
def test_remove_outlier_many(ctx, many_batches, k):
    """clouds of unequal size in one launch, empty ones at the front, inside and at the end: every cloud's keep mask"""
    name, radius, min_points, clouds = many_batches[k]
    off = np.r_[0, np.cumsum([len(p) for p in clouds])].astype(np.int32)
    pts = np.ascontiguousarray(np.concatenate(clouds), F)
    keep = np.full(len(pts), 7, np.uint8)
    with ctx.lock:
        ctx._check(ctx.lib.sfe_remove_outlier_many(ctx.handle, L.ptr(pts, C.c_float), L.ptr(off, C.c_int32), len(clouds),
                                                   float(radius), int(min_points), L.ptr(keep, C.c_uint8)))
    assert set(np.unique(keep)) <= {0, 1}
    bad = []
    for i, p in enumerate(clouds):
        if len(p):
            rows, want = E.ref_outlier(p, radius, min_points)
            got = keep[off[i]:off[i + 1]].astype(bool)
            if not np.array_equal(got, want) or not np.array_equal(E.bits(p[got]), E.bits(rows)):
                bad.append((name, i, len(p)))
    assert not bad, bad
