"""GPU: the cloud functions of ``pcl`` on N x 3 clouds (sfe_pcl3.hip) against the numpy restatement of their rules
(tests/pcl3_ref.py), bit for bit; a cloud with z = 0 against the existing 2-D calls; what stays refused.

Sizes: the reference cloud of match crosses one LDS tile (2048 points) and the queries are no multiple of 64; the outlier
filter and the larger downsample cross a tile too; the smaller ones stay inside one workgroup.
"""
import numpy as np
import pytest

import pcl3_ref
from sonar_slam_amd import pcl

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _uniform(seed, n, lo=0.0, hi=10.0):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(np.float32)


def _clustered(seed, n, n_dup):
    """clusters in a 10 x 10 x 4 box (not a cube: the root radius comes from x), a fifth of the points spread evenly, the
    last n_dup rows exact copies of the first ones; the box corners are pinned so the tree depth is known"""
    rng = np.random.default_rng(seed)
    box = np.array([10.0, 10.0, 4.0])
    centres = rng.uniform(0.5, 0.9, (max(n // 10, 1), 3)) * box
    p = centres[rng.integers(0, len(centres), n)] + rng.normal(0, 0.12, (n, 3))
    spread = rng.random(n) < 0.2
    p[spread] = rng.uniform(0, 1, (int(spread.sum()), 3)) * box
    p = np.clip(p, 0, box).astype(np.float32)
    p[0], p[1] = (0, 0, 0), box
    p[n - n_dup:] = p[2:2 + n_dup]
    return p


# ---- match ----
@pytest.fixture(scope="module")
def match_case():
    ref = _uniform(11, 2085)
    ref[:400] = np.round(ref[:400] * 2) / 2          # a coarse lattice: equal distances from lattice queries
    ref[1500:] = ref[:585]                           # exact duplicates, most of them behind the tile boundary
    pts = _uniform(12, 130, -1.0, 11.0)
    pts[:20] = ref[390:410]                          # queries on reference points (d2 = 0, twice)
    pts[20:40] = np.round(pts[20:40] * 2) / 2
    return ref, pts


@pytest.mark.parametrize("knn", [1, 3])
def test_match(ctx, match_case, knn):
    ref, pts = match_case
    ids_r, d2_r = pcl3_ref.match_knn(ref, pts, knn, 0.75)
    # the cases the comparison is about occur: an index tie decided, and a query with fewer than knn neighbours
    dup_of = {i: i + 1500 for i in range(585)}
    if knn == 1:
        assert any(int(i) in dup_of for i in ids_r[0])               # the nearest point has a copy at a higher index
    else:
        tie = np.isfinite(d2_r[1:]) & (d2_r[1:] == d2_r[:-1])
        assert tie.any() and (ids_r[1:][tie] > ids_r[:-1][tie]).all()
    assert (ids_r[-1] == -1).any() and (ids_r[-1] >= 0).any()
    if knn == 3:
        assert ((ids_r[0] >= 0) & (ids_r[2] == -1)).any()            # some, but fewer than knn
    ids, d2 = pcl.match(ref, pts, knn, 0.75, ctx=ctx)
    assert ids.shape == (knn, 130) and ids.dtype == np.int32 and d2.dtype == np.float32
    assert np.array_equal(ids, ids_r)
    assert np.array_equal(_bits(d2), _bits(d2_r))


def test_match_knn_beyond_the_reference_raises(ctx):
    with pytest.raises(RuntimeError, match="exceeds the 2 points"):
        pcl.match(np.zeros((2, 3), np.float32), np.zeros((5, 3), np.float32), 3, 1.0, ctx=ctx)


# ---- remove_outlier ----
def test_remove_outlier(ctx):
    pts = _uniform(21, 2100)
    pts[2000:] = pts[:100]
    want, keep = pcl3_ref.remove_outlier(pts, 0.7, 3, return_mask=True)
    assert 0.2 * len(pts) <= keep.sum() <= 0.8 * len(pts)
    got = pcl.remove_outlier(pts, 0.7, 3, ctx=ctx)
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.array_equal(_bits(got), _bits(want))


# ---- knn_density ----
def test_knn_density(ctx):
    pts = _clustered(31, 300, 50)
    pts[100:106] = pts[99]                           # more coincident points than knn: r = 0, an infinite density
    want = pcl3_ref.knn_density(pts, 5)
    assert np.isinf(want).any() and np.isfinite(want).sum() > 200
    got = pcl.knn_density(pts, 5, ctx=ctx)
    assert got.shape == (300,) and np.array_equal(_bits(got), _bits(want))


def test_max_density_filter_keeps_the_width(ctx):
    pts = _clustered(32, 300, 20)
    dens = pcl3_ref.knn_density(pts, 4)
    cap = float(np.median(dens[np.isfinite(dens)]))
    pcl.srand(7)
    out, desc = pcl.max_density_filter(pts, np.arange(300, dtype=np.float32)[:, None], 4, cap, ctx=ctx)
    assert out.shape[1] == 3 and 0 < len(out) < 300
    assert np.array_equal(_bits(out), _bits(pts[desc[:, 0].astype(int)]))       # rows of the input, in input order
    assert (np.diff(desc[:, 0]) > 0).all() and (dens[desc[:, 0].astype(int)] <= cap).sum() == (dens <= cap).sum()


# ---- downsample ----
@pytest.fixture(scope="module", params=[300, 3000])
def ds_case(request):
    n = request.param
    pts = _clustered(40 + n, n, n // 6)
    info = {}
    out, idx = pcl3_ref.downsample(pts, 0.35, info)
    return pts, out, idx, info


def test_downsample(ctx, ds_case):
    pts, want, idx, info = ds_case
    sizes = np.array([len(leaf) for leaf in info["leaves"]])
    assert 4 <= info["depth"] <= 6
    assert (sizes >= 2).sum() * 4 >= len(sizes)                      # at least a quarter of the leaves are no singletons
    assert any(t >= 2 for t in info["ties"])                         # a centroid-distance tie, decided for the first point
    got = pcl.downsample(pts, 0.35, ctx=ctx)
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.array_equal(_bits(got), _bits(want))


def test_downsample_descriptors_follow_the_indices(ctx, ds_case):
    pts, want, idx, _ = ds_case
    desc = np.c_[np.arange(len(pts)), -np.arange(len(pts))].astype(np.float32)
    got, got_desc = pcl.downsample(pts, desc, 0.35, ctx=ctx)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(got_desc, desc[idx])


def test_downsample_resolution_zero_splits_to_the_cap(ctx):
    pts = _uniform(51, 64, -3.0, 3.0)
    pts[60:] = pts[:4]
    info = {}
    want, idx = pcl3_ref.downsample(pts, 0.0, info)
    assert info["depth"] == pcl3_ref.MAX_LEVELS and len(want) == 60
    got, got_desc = pcl.downsample(pts, np.arange(64, dtype=np.float32)[:, None], 0.0, ctx=ctx)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(got_desc[:, 0].astype(np.int32), idx)


# ---- z = 0: the existing 2-D calls with a zero column appended ----
@pytest.fixture(scope="module")
def flat():
    p = _clustered(61, 2300, 300)
    q = _clustered(62, 130, 10)
    p[:, 2] = 0
    q[:, 2] = 0
    return p, q


def _z0(xy):
    return np.c_[xy, np.zeros(len(xy), np.float32)].astype(np.float32)


@pytest.mark.parametrize("knn", [1, 3])
def test_flat_match_is_the_2d_match(ctx, flat, knn):
    p, q = flat
    ids3, d3 = pcl.match(p, q, knn, 0.2, ctx=ctx)
    ids2, d2 = pcl.match(p[:, :2], q[:, :2], knn, 0.2, ctx=ctx)
    assert (ids2 == -1).any() and (ids2 >= 0).any()
    assert np.array_equal(ids3, ids2) and np.array_equal(_bits(d3), _bits(d2))


def test_flat_remove_outlier_is_the_2d_filter(ctx, flat):
    p, _ = flat
    want = pcl.remove_outlier(p[:, :2], 0.2, 8, ctx=ctx)
    assert 0 < len(want) < len(p)
    assert np.array_equal(_bits(pcl.remove_outlier(p, 0.2, 8, ctx=ctx)), _bits(_z0(want)))


def test_flat_knn_density_is_the_2d_density(ctx, flat):
    _, q = flat
    assert np.array_equal(_bits(pcl.knn_density(q, 5, ctx=ctx)), _bits(pcl.knn_density(q[:, :2], 5, ctx=ctx)))


def test_flat_downsample_is_the_2d_downsample(ctx, flat):
    p, _ = flat
    desc = np.arange(len(p), dtype=np.float32)[:, None]
    want, want_desc = pcl.downsample(p[:, :2], desc, 0.35, ctx=ctx)
    assert len(want) < len(p)
    got, got_desc = pcl.downsample(p, desc, 0.35, ctx=ctx)
    assert np.array_equal(_bits(got), _bits(_z0(want))) and np.array_equal(got_desc, want_desc)
    assert np.array_equal(_bits(pcl.downsample(p, 0.35, ctx=ctx)), _bits(_z0(pcl.downsample(p[:, :2], 0.35, ctx=ctx))))


# ---- edges and refusals ----
def test_empty_clouds_come_back_unchanged(ctx):
    e = np.zeros((0, 3), np.float32)
    assert pcl.remove_outlier(e, 1.0, 2, ctx=ctx).shape == (0, 3)
    assert pcl.downsample(e, 0.5, ctx=ctx).shape == (0, 3)
    assert pcl.max_density_filter(e, 3, 1.0, ctx=ctx).shape == (0, 3)
    ids, d2 = pcl.match(np.ones((3, 3), np.float32), e, 1, 1.0, ctx=ctx)
    assert ids.shape == (1, 0) and d2.shape == (1, 0)


def test_icp_on_3d_clouds_stays_refused(ctx):
    from sonar_slam_amd import icp_config
    icp = pcl.ICP(ctx)
    icp.setParams(icp_config.shipped_params())
    cloud = _uniform(71, 50)
    with pytest.raises(NotImplementedError, match="N x 3 clouds"):
        icp.compute(cloud, cloud, np.eye(3, dtype=np.float32))
    with pytest.raises(NotImplementedError, match="4 x 4 guesses"):
        icp.compute(cloud[:, :2], cloud[:, :2], np.eye(4, dtype=np.float32))
