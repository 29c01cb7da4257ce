"""The references of tests/store_ref.py against the oracle and against what the existing store tests assert, and the constructed
inputs of tests/test_gpu_store_edges.py against what they are built to hold.  No GPU."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import oracle  # noqa: E402
import store_ref as R  # noqa: E402
from sonar_slam_amd.replay import FrontEnd  # noqa: E402


def test_match_first_equals_the_oracle_match_across_tile_sizes():
    rng = np.random.default_rng(21)
    for nt, ns in ((2047, 255), (2048, 256), (2049, 257), (1, 5), (300, 513)):
        tgt, src = R.random_cloud(rng, nt), R.random_cloud(rng, ns)
        ids, d2 = R.match_first(tgt, src, 0.4)
        want_ids, want_d2 = oracle.match(tgt, src, 0.4)
        assert np.array_equal(ids, want_ids.reshape(-1)) and np.array_equal(d2, want_d2.reshape(-1))
        assert int(np.sum(ids != -1)) == oracle.overlap(src, tgt, np.eye(3), 0.4, f64_points=False)
        if nt > 1000:
            assert 0 < int(np.sum(ids != -1)) < ns       # the radius decides something


def test_match_first_without_a_finite_distance_and_on_the_radius():
    assert R.match_first(np.zeros((0, 2)), np.zeros((3, 2)), 0.5)[0].tolist() == [-1, -1, -1]
    assert R.match_first(np.zeros((3, 2)), np.zeros((0, 2)), 0.5)[0].tolist() == []
    t, _, q, bad = R.nonfinite_inputs()
    ids, _ = R.match_first(t, q, 0.5)
    good = np.setdiff1d(np.arange(len(q)), bad)
    assert np.all(ids[bad] == -1) and np.array_equal(ids[good], good) and len(bad) == 9
    t, _, q, want = R.radius_inputs()
    ids, d2 = R.match_first(t, q, 0.5)
    assert (ids != -1).tolist() == [True] * 4 + [False] * 4 and want == 4
    assert np.all(ids[:4] == R.TILE) and np.all(d2[:4] == np.float32(0.25))
    assert oracle.match(t, q, 0.5)[0].reshape(-1).tolist() == ids.tolist()


def test_match_first_takes_the_lowest_index_among_equals():
    t, keys, q, n_keys, want, want_ov = R.tie_inputs()
    ids, _ = R.match_first(t, q, 0.5)
    lows, highs = [p[0] for p in R.TIE_PAIRS], [p[1] for p in R.TIE_PAIRS]
    for lo, hi in R.TIE_PAIRS:
        assert np.array_equal(t[lo], t[hi]) and keys[lo] != keys[hi] and (lo // R.TILE != hi // R.TILE) == (lo == R.TILE - 1)
        assert int(np.sum(ids == lo)) == 30
    assert not np.isin(ids, highs).any() and np.isin(ids, lows).sum() == 60
    hist, ov = R.match_keys(t, keys, q, 0.5, n_keys)
    assert np.array_equal(hist, want) and ov == want_ov == len(q) and hist[[2, 4]].tolist() == [0, 0]
    assert np.array_equal(oracle.match(t, q, 0.5)[0].reshape(-1), ids)       # the oracle's documented choice is the same
    # both source blocks hold queries on both pairs
    for blk in (ids[:R.BLOCK], ids[R.BLOCK:]):
        assert np.isin(lows, blk).all()


def test_designated_neighbours_are_the_only_match_of_their_queries():
    t, keys, q, n_keys, want, want_ov = R.designated_inputs()
    assert R.DESIGNATED == (2047, 2048, 4095, 4096) and len(q) > R.BLOCK
    ids, d2 = R.match_first(t, q, 0.5)
    for j, i in enumerate(R.DESIGNATED):
        assert int(np.sum(keys == 1 + j)) == 1 and keys[i] == 1 + j and int(np.sum(ids == i)) == 20
    # unique: the second nearest target of every matched query is far beyond the radius, and so is all of an unmatched one's
    d = np.sort(((q[:, None, :].astype(np.float64) - t[None, :, :]) ** 2).sum(axis=2), axis=1)
    assert np.all(d[ids >= 0, 1] > 9.0) and np.all(d[ids < 0, 0] == 8.0)
    hist, ov = R.match_keys(t, keys, q, 0.5, n_keys)
    assert np.array_equal(hist, want) and ov == want_ov and int(np.sum(ids == -1)) == 80


def test_match_keys_leaves_large_keys_out_of_the_histogram_only():
    t = R.lattice(10)
    keys = np.arange(10, dtype=np.int32)
    hist, ov = R.match_keys(t, keys, t, 0.5, 4)
    assert hist.tolist() == [1, 1, 1, 1] and ov == 10
    hist, ov = R.match_keys(t, keys, t, 0.5, 0)
    assert hist.tolist() == [] and ov == 10


def test_append_layout_reproduces_the_offsets_the_store_test_asserts():
    """tests/test_gpu_store.py::test_put_read_meta_truncate: four puts into a pool of 10 000, then (after a truncate to two
    slots) a cloud of 1300 at 700, a cloud of 9000 that does not fit, and one point behind it at 2000"""
    off, cnt, top = R.append_layout(0, [700, 0, 1, 1300], 1300, 10000)
    assert off.tolist() == [0, 700, 700, 701] and cnt.tolist() == [700, 0, 1, 1300] and top == 2001
    off, cnt, top = R.append_layout(700, [1300], 1300, 10000)
    assert off.tolist() == [700] and top == 2000
    off, cnt, top2 = R.append_layout(top, [9000], 9000, 10000)
    assert off.tolist() == [-1] and cnt.tolist() == [R.OVERFLOW] and top2 == 2000
    off, cnt, top3 = R.append_layout(top2, [1], 1, 10000)
    assert off.tolist() == [2000] and cnt.tolist() == [1] and top3 == 2001


def test_append_layout_clamps_keeps_negative_counts_and_stops_at_the_first_overflow():
    off, cnt, top = R.append_layout(5, [7, -1, 0, 4, 2, 0, -1, 1], 4, 16)
    #                                   4   0  0  4  (5 + 8 + 2 = 15 <= 16)  0  -1  1
    assert off.tolist() == [5, 9, 9, 9, 13, 15, 15, 15] and cnt.tolist() == [4, -1, 0, 4, 2, 0, -1, 1] and top == 16
    off, cnt, top = R.append_layout(5, [7, -1, 0, 4, 2, 0, -1, 1], 4, 14)
    assert off.tolist() == [5, 9, 9, 9, -1, -1, -1, -1] and cnt.tolist() == [4, -1, 0, 4, -3, -3, -3, -3] and top == 13
    off, cnt, top = R.append_layout(0, [], 4, 14)
    assert len(off) == 0 and top == 0


def test_compact_and_bbox():
    p = np.float32([[1, -2], [-3, 4], [5, 0]])
    pts, keys = R.compact(p, np.int32([7, 8, 9]), [1, 0, 1])
    assert pts.tolist() == [[1, -2], [5, 0]] and keys.tolist() == [7, 9]
    assert R.bbox(p).tolist() == [-3, -2, 5, 4]
    assert R.key_counts([0, 3, 3, 9], 4).tolist() == [1, 0, 0, 2]


def test_the_field_of_view_inputs_lose_no_point_to_the_screen():
    jobs = R.fov_inputs()
    assert [len(j[0]) for j in jobs] == list(R.FOV_SIZES) and [len(j[2]) for j in jobs] == list(R.FOV_FRAMES_PER_JOB)
    decided = 0
    for pts, keys, frames, rb, bb in jobs:
        assert not R.fov_near_a_bound(pts, frames, bb).any()
        sel = FrontEnd._fov_numpy(pts, frames, rb, bb)
        if len(frames) == 0:
            assert not sel.any()
        elif len(pts) > 200:
            assert 0 < sel.sum() < len(pts)               # the gate decides something
            assert keys[sel].max() >= R.FOV_N_KEYS         # ... and selects keys the histogram has no bin for
            decided += 1
    assert decided == 3
    # the screen itself: a point exactly on a bound, and one 2e-5 (relative) inside it
    from sonar_slam_amd.pose2 import Pose2
    eye = Pose2(0.0, 0.0, 0.0)
    p = np.array([[np.cos(0.7), np.sin(0.7)], [np.cos(0.7 * (1 - 2e-5)), np.sin(0.7 * (1 - 2e-5))]])
    assert R.fov_near_a_bound(p, [eye], [0.7]).tolist() == [True, False]


def test_the_range_of_the_field_of_view_gate_is_exact_in_the_reference():
    """(3, 4) is at range exactly 5: outside a bound of 5.0, inside the next double above it"""
    from sonar_slam_amd.pose2 import Pose2
    eye = Pose2(0.0, 0.0, 0.0)
    p = np.float32([[3, 4], [-3, 4], [4, -3], [0, 5]])
    assert not FrontEnd._fov_numpy(p, [eye], [5.0], [3.0]).any()
    assert FrontEnd._fov_numpy(p, [eye], [np.nextafter(5.0, 6.0)], [3.0]).all()
    assert FrontEnd._fov_numpy(p, [eye], [np.nextafter(5.0, 6.0)], [1.0]).tolist() == [True, False, True, False]
