"""Host side of the N x 3 cloud functions of ``pcl`` (match, remove_outlier, knn_density, downsample):

* the numpy restatement the GPU tests compare against (tests/pcl3_ref.py), restricted to z = 0, equals the oracle's 2-D
  functions on the same (x, y), bit for bit: the third term of d2 is +0, a constant z gives every point the same z bit
  at every octree level, so the leaves and their order are the quadtree's;
* the argument checks of pcl.py raise before any device call (none of these needs a GPU).
"""
import numpy as np
import pytest

import oracle
import pcl3_ref
from sonar_slam_amd import pcl


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _xy(seed, n, dup):
    """clustered (x, y) with exact duplicates and a few coordinates on a coarse lattice (equal distances)"""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0, 10, (max(n // 12, 1), 2))
    xy = (centres[rng.integers(0, len(centres), n)] + rng.normal(0, 0.25, (n, 2))).astype(np.float32)
    xy[: n // 4] = np.round(xy[: n // 4] * 4) / 4
    xy[n - dup:] = xy[:dup]
    return xy


def _z0(xy):
    return np.c_[xy, np.zeros(len(xy), np.float32)].astype(np.float32)


@pytest.fixture(scope="module")
def clouds():
    return _xy(1, 420, 60), _xy(2, 90, 10)


@pytest.mark.parametrize("knn", [1, 3])
def test_match_z0_is_the_oracles_2d_match(clouds, knn):
    ref, pts = clouds
    ids, d2 = pcl3_ref.match_knn(_z0(ref), _z0(pts), knn, 0.3)
    ids_o, d2_o = oracle.match_knn(ref, pts, knn, 0.3)
    assert (ids == -1).any() and (ids >= 0).all(axis=0).any()
    assert np.array_equal(ids, ids_o) and np.array_equal(_bits(d2), _bits(d2_o))
    if knn == 1:
        ids_1, d2_1 = oracle.match(ref, pts, 0.3)
        assert np.array_equal(ids, ids_1) and np.array_equal(_bits(d2), _bits(d2_1))
        ids_m, d2_m = pcl3_ref.match(_z0(ref), _z0(pts), 0.3)
        assert np.array_equal(ids, ids_m) and np.array_equal(_bits(d2), _bits(d2_m))


def test_remove_outlier_z0_is_the_oracles_2d_filter(clouds):
    ref, _ = clouds
    got = pcl3_ref.remove_outlier(_z0(ref), 0.35, 6)
    want = oracle.remove_outlier(ref, 0.35, 6)
    assert 0.2 * len(ref) < len(want) < 0.8 * len(ref)
    assert np.array_equal(_bits(got), _bits(_z0(want)))


def test_knn_density_z0_is_the_oracles_2d_density(clouds):
    ref, _ = clouds
    got = pcl3_ref.knn_density(_z0(ref), 5)
    assert np.array_equal(_bits(got), _bits(oracle.knn_density(ref, 5)))
    with pytest.raises(RuntimeError):
        pcl3_ref.knn_density(_z0(ref[:3]), 4)


@pytest.mark.parametrize("resolution", [0.3, 0.7, 2.5])
def test_downsample_z0_is_the_oracles_2d_octree(clouds, resolution):
    ref, _ = clouds
    info = {}
    got, idx = pcl3_ref.downsample(_z0(ref), resolution, info)
    want, idx_o = oracle.downsample(ref, resolution, return_index=True)
    assert any(len(leaf) >= 2 for leaf in info["leaves"]) and 2 <= info["depth"] <= pcl3_ref.MAX_LEVELS
    assert np.array_equal(idx, idx_o)
    assert np.array_equal(_bits(got), _bits(_z0(want)))


def test_downsample_cuts_the_tree_at_the_key_capacity():
    """resolution 0 never ends the splitting by size: coincident points share a leaf at the cap, the others end alone"""
    pts = np.random.default_rng(3).uniform(-1, 1, (12, 3)).astype(np.float32)
    pts[9:] = pts[:3]
    info = {}
    out, idx = pcl3_ref.downsample(pts, 0.0, info)
    assert info["depth"] == pcl3_ref.MAX_LEVELS and len(out) == 9
    assert sorted(idx.tolist()) == list(range(9))              # of two coincident points the first one is the medoid


# ---- pcl.py: refusals that must not need a device ----
@pytest.mark.parametrize("shape", [(5, 4), (5, 1), (6,), (2, 3, 3)])
def test_a_width_other_than_2_or_3_is_a_type_error(shape):
    bad = np.zeros(shape, np.float32)
    ok = np.zeros((4, 3), np.float32)
    for call in (lambda: pcl.match(ok, bad, 1, 1.0), lambda: pcl.match(bad, ok, 1, 1.0),
                 lambda: pcl.remove_outlier(bad, 1.0, 2), lambda: pcl.downsample(bad, 0.5),
                 lambda: pcl.downsample(bad, np.zeros((len(bad), 1), np.float32), 0.5),
                 lambda: pcl.knn_density(bad, 1), lambda: pcl.max_density_filter(bad, 1, 1.0)):
        with pytest.raises(TypeError, match="N x 2 or N x 3"):
            call()


def test_match_refuses_clouds_of_different_widths():
    a2, a3 = np.zeros((4, 2), np.float32), np.zeros((4, 3), np.float32)
    with pytest.raises(RuntimeError, match=r"N x 2 .* N x 3"):
        pcl.match(a2, a3, 1, 1.0)
    with pytest.raises(RuntimeError, match=r"N x 3 .* N x 2"):
        pcl.match(a3, a2, 1, 1.0)


def test_downsample_refuses_a_descriptor_count_mismatch():
    with pytest.raises(TypeError, match="4 descriptors for 5 points"):
        pcl.downsample(np.zeros((5, 3), np.float32), np.zeros((4, 2), np.float32), 0.5)


def test_knn_density_refuses_more_neighbours_than_points():
    with pytest.raises(RuntimeError, match="more points than available"):
        pcl.knn_density(np.zeros((3, 3), np.float32), 4)


def test_empty_clouds_pass_through_downsample_and_max_density_filter():
    e = np.zeros((0, 3), np.float32)
    out = pcl.downsample(e, 0.5)
    assert out.shape == (0, 3) and out.dtype == np.float32
    out, desc = pcl.downsample(e, np.zeros((0, 2), np.float32), 0.5)
    assert out.shape == (0, 3) and desc.shape == (0, 2)
    assert pcl.max_density_filter(e, 3, 1.0).shape == (0, 3)
