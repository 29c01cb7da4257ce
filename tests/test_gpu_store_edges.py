"""The keyframe store's kernels (csrc/sfe_store.hip, cost_bbox_kernel of csrc/sfe_cost.hip) where they change behaviour: the
1024-frame passes of the commit kernel, the 2048-target tiles and 256-source blocks of the matching kernels, the 1024-point chunks
and 64-lane ballots of the compaction, jobs whose blocks all return early, empty clouds, a full pool.  Every cloud goes in through
put / put_keys / put_batch_dev / set_selection, so its content and order are known; every expectation is exact (integers and
float32 copies), against tests/store_ref.py, the oracle and FrontEnd._fov_numpy.  tests/test_store_ref_host.py checks those
references and the constructed inputs on the CPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import oracle  # noqa: E402
import store_ref as R  # noqa: E402
from sonar_slam_amd import _lib  # noqa: E402
from sonar_slam_amd import store as st  # noqa: E402
from sonar_slam_amd.pose2 import Pose2  # noqa: E402
from sonar_slam_amd.replay import FrontEnd  # noqa: E402

pytestmark = pytest.mark.gpu

EYE6 = st.pose_T6(np.eye(3))
DTYPES = pytest.mark.parametrize("flags", [0, st.F32_POINTS], ids=["f64_points", "f32_points"])


def _cloud(rng, n):
    return np.c_[rng.uniform(1, 29, n), rng.uniform(-20, 20, n)].astype(np.float32)


def _offset(s, h):
    return int(s.meta(h, 1)[1][0])


# ---- append / commit / rewind -------------------------------------------------------------------------------------------------
CAP, N_FRAMES, FIRST_FULL, N_BEFORE = 4, 1030, 517, 5


def _batch():
    """1030 frames in the [frame][cap] float2 layout of the resident filters + counts[frame]: more than one 1024-frame pass of
    the commit kernel, counts above the stride (7 -> 4), below zero and zero, on both sides of the pass boundary"""
    rng = np.random.default_rng(31)
    counts = rng.choice([-1, 0, 1, 2, 3, 4, 7], N_FRAMES).astype(np.int32)
    counts[[0, 1, 2, 3]] = [7, -1, 0, 4]
    counts[510], counts[FIRST_FULL] = 2, 3
    counts[1020:1030] = [3, 7, -1, 0, 4, 7, 1, -1, 2, 3]
    clouds = rng.uniform(-30, 30, (N_FRAMES, CAP, 2)).astype(np.float32)
    return clouds, counts


def _append(ctx, s, clouds, counts, flags=0):
    d_clouds, d_counts = ctx.alloc(clouds.nbytes), ctx.alloc(counts.nbytes)
    try:
        d_clouds.upload(clouds)
        d_counts.upload(counts)
        hs = s.put_batch_dev(d_clouds, d_counts, len(counts), clouds.shape[1], stamps=np.arange(len(counts)) + 50, flags=flags)
        s.meta()        # (the append is enqueue-only: drained before the inputs go)
    finally:
        d_clouds.free()
        d_counts.free()
    return hs


def _stored_equal(s, first, clouds, cnt, flags=0):
    """every cloud with a count above 0 reads back as the first n points of its frame"""
    live = np.nonzero(cnt > 0)[0]
    got = s.read_many(first + live)
    for f, g in zip(live, got):
        want = clouds[f, :cnt[f]] * (np.float32([1, -1]) if flags & st.NEGATE_Y else np.float32([1, 1]))
        assert np.array_equal(g, want), f
    return len(live)


def _store_with_batch(ctx, capacity, flags=0):
    clouds, counts = _batch()
    s = st.CloudStore(ctx, capacity_points=capacity, max_clouds=2048)
    before = _cloud(np.random.default_rng(30), N_BEFORE)
    assert s.put(before, stamp=7) == 0
    hs = _append(ctx, s, clouds, counts, flags)
    assert hs.tolist() == list(range(1, 1 + N_FRAMES)) and len(s) == 1 + N_FRAMES
    return s, before, clouds, counts


@pytest.mark.parametrize("flags", [0, st.NEGATE_Y], ids=["as_is", "negate_y"])
def test_append_of_1030_frames_with_clamped_and_negative_counts(ctx, flags):
    s, before, clouds, counts = _store_with_batch(ctx, 1 << 13, flags)
    stamps, off, cnt = s.meta(1, N_FRAMES)
    want_off, want_cnt, top = R.append_layout(N_BEFORE, counts, CAP, s.capacity_points)
    assert np.array_equal(off, want_off) and np.array_equal(cnt, want_cnt) and stamps.tolist() == list(range(50, 50 + N_FRAMES))
    assert np.all(cnt[counts == 7] == CAP) and np.all(cnt[counts == -1] == -1) and np.all(off >= N_BEFORE)
    assert (counts[1021], counts[1025]) == (7, 7) and off[1029] > off[1023] > off[1020]   # the carry into the second pass
    assert _stored_equal(s, 1, clouds, cnt, flags) > 600
    assert np.array_equal(s.read(0), before) and s.meta(0, 1)[1].tolist() == [0]
    h = s.put(before[:1])
    assert _offset(s, h) == top and np.array_equal(s.read(h), before[:1])
    s.close()


def _overflowing_store(ctx):
    """the batch into a pool in which frame 517 (of 3 points) is the first that does not fit, by one point"""
    _, counts = _batch()
    open_off, open_cnt, _ = R.append_layout(N_BEFORE, counts, CAP, 1 << 40)
    capacity = int(open_off[FIRST_FULL]) + 3 - 1
    s, before, clouds, counts = _store_with_batch(ctx, capacity)
    return s, before, clouds, counts, open_off, open_cnt


def test_append_that_overflows_in_the_middle_of_the_batch(ctx):
    s, before, clouds, counts, open_off, open_cnt = _overflowing_store(ctx)
    _, off, cnt = s.meta(1, N_FRAMES)
    want_off, want_cnt, top = R.append_layout(N_BEFORE, counts, CAP, s.capacity_points)
    assert np.array_equal(off, want_off) and np.array_equal(cnt, want_cnt)
    assert np.all(off[FIRST_FULL:] == -1) and np.all(cnt[FIRST_FULL:] == R.OVERFLOW) and top == open_off[FIRST_FULL]
    assert np.array_equal(off[:FIRST_FULL], open_off[:FIRST_FULL]) and np.array_equal(cnt[:FIRST_FULL], open_cnt[:FIRST_FULL])
    assert _stored_equal(s, 1, clouds, np.where(np.arange(N_FRAMES) < FIRST_FULL, cnt, 0)) > 300
    assert np.array_equal(s.read(0), before)
    with pytest.raises(_lib.SonarFEError):
        s.read(1 + FIRST_FULL)
    # the level stopped where frame 517 would have begun: two points are left, a cloud of one lands there
    h = s.put(before[:1])
    assert h == 1 + N_FRAMES and _offset(s, h) == open_off[FIRST_FULL] and np.array_equal(s.read(h), before[:1])
    assert _stored_equal(s, 1, clouds, np.where(np.arange(N_FRAMES) < FIRST_FULL, cnt, 0)) > 300
    s.close()


def test_append_that_fills_the_pool_exactly(ctx):
    _, counts = _batch()
    _, _, open_top = R.append_layout(N_BEFORE, counts, CAP, 1 << 40)
    s, before, clouds, counts = _store_with_batch(ctx, open_top)
    _, off, cnt = s.meta(1, N_FRAMES)
    want_off, want_cnt, top = R.append_layout(N_BEFORE, counts, CAP, open_top)
    assert np.array_equal(off, want_off) and np.array_equal(cnt, want_cnt) and not np.any(cnt == R.OVERFLOW)
    assert top == s.capacity_points and off[-1] + cnt[-1] == s.capacity_points
    assert _stored_equal(s, 1, clouds, cnt) > 600
    h = s.put(np.zeros((0, 2), np.float32))            # nothing is left but room for nothing
    assert _offset(s, h) == top and s.counts([h])[0] == 0
    h = s.put(before[:1])
    assert _offset(s, h) == -1 and s.counts([h])[0] == R.OVERFLOW
    s.close()


def test_truncate_over_overflowed_slots_keeps_the_level_and_over_a_stored_cloud_rewinds_to_it(ctx):
    s, before, clouds, counts, open_off, open_cnt = _overflowing_store(ctx)
    s.truncate(1 + 600)                                 # every dropped slot had overflowed
    h = s.put(before[:1])
    assert h == 1 + 600 and _offset(s, h) == open_off[FIRST_FULL] and np.array_equal(s.read(h), before[:1])
    assert s.meta(1 + FIRST_FULL, 600 - FIRST_FULL)[2].tolist() == [R.OVERFLOW] * (600 - FIRST_FULL)
    s.truncate(1 + 510)                                 # frame 510 holds two points, frames 517 .. 599 behind it overflowed
    assert open_cnt[510] == 2
    h = s.put(before[:2])
    assert h == 1 + 510 and _offset(s, h) == open_off[510] and np.array_equal(s.read(h), before[:2])
    live = np.where(np.arange(N_FRAMES) < 510, open_cnt, 0)
    assert _stored_equal(s, 1, clouds[:510], live[:510]) > 300 and np.array_equal(s.read(0), before)
    s.close()


# ---- overlap and match_keys ---------------------------------------------------------------------------------------------------
@DTYPES
def test_overlap_and_match_keys_across_tile_and_block_sizes(ctx, flags):
    rng = np.random.default_rng(41)
    s = st.CloudStore(ctx, capacity_points=1 << 16, max_clouds=64)
    pose = Pose2(0.3, -0.2, 0.05)
    T6, n_keys, max_dist = st.pose_T6(pose), 6, 0.4
    cases = []
    for nt, ns in R.SIZE_PAIRS:
        tgt, keys, src = R.random_cloud(rng, nt), rng.integers(0, n_keys, nt).astype(np.int32), R.random_cloud(rng, ns)
        cases.append((s.put(src), s.put_keys(tgt, keys), src, tgt, keys))
    pairs = [(c[0], c[1]) for c in cases]
    got = s.overlap(pairs, [T6] * len(pairs), max_dist, flags=flags)
    hists, ovs = s.match_keys_many([p[0] for p in pairs], [T6] * len(pairs), [p[1] for p in pairs], max_dist, n_keys, flags=flags)
    for (hs, ht, src, tgt, keys), ov, hist_m, ov_m in zip(cases, got, hists, ovs):
        moved = oracle.transform_points(src, pose.matrix(), f64_points=not flags)
        want_hist, want_ov = R.match_keys(tgt, keys, moved, max_dist, n_keys)
        assert want_ov == oracle.overlap(src, tgt, pose.matrix(), max_dist, f64_points=not flags)
        assert ov == want_ov and ov_m == want_ov and np.array_equal(hist_m, want_hist), (len(tgt), len(src))
        hist, ov1 = s.match_keys(hs, T6, ht, max_dist, n_keys, flags=flags)
        assert ov1 == want_ov and np.array_equal(hist, want_hist), (len(tgt), len(src))
        if len(tgt) > 2000 and len(src) > 200:
            assert 0 < want_ov < len(src)
    s.close()


def _match_case(ctx, flags, t, keys, q, n_keys, max_dist=0.5):
    s = st.CloudStore(ctx, capacity_points=1 << 14, max_clouds=8)
    ht, hq = s.put_keys(t, keys), s.put(q)
    hist, ov = s.match_keys(hq, EYE6, ht, max_dist, n_keys, flags=flags)
    ov2 = int(s.overlap([(hq, ht)], [EYE6], max_dist, flags=flags)[0])
    s.close()
    return hist, ov, ov2


@DTYPES
def test_nearest_neighbours_on_tile_edges_credit_their_own_key(ctx, flags):
    t, keys, q, n_keys, want, want_ov = R.designated_inputs()
    hist, ov, ov2 = _match_case(ctx, flags, t, keys, q, n_keys)
    assert hist.tolist() == want.tolist() == [140, 20, 20, 20, 20] and ov == ov2 == want_ov


@DTYPES
def test_a_tie_across_the_tile_edge_goes_to_the_lower_index(ctx, flags):
    t, keys, q, n_keys, want, want_ov = R.tie_inputs()
    hist, ov, ov2 = _match_case(ctx, flags, t, keys, q, n_keys)
    assert hist.tolist() == want.tolist() == [210, 30, 0, 30, 0] and ov == ov2 == want_ov


@DTYPES
def test_a_distance_exactly_on_the_radius_counts_and_the_next_float_does_not(ctx, flags):
    t, keys, q, want_ov = R.radius_inputs()
    hist, ov, ov2 = _match_case(ctx, flags, t, keys, q, 2)
    assert hist.tolist() == [0, 4] and ov == ov2 == want_ov == 4
    hist, ov, ov2 = _match_case(ctx, flags, t, keys, q[4:], 2)
    assert hist.tolist() == [0, 0] and ov == ov2 == 0


@DTYPES
def test_sources_with_nan_or_infinite_coordinates_never_count(ctx, flags):
    t, keys, q, bad = R.nonfinite_inputs()
    good = np.setdiff1d(np.arange(len(q)), bad)
    hist, ov, ov2 = _match_case(ctx, flags, t, keys, q, 6)
    assert ov == ov2 == len(good) == 248 and np.array_equal(hist, R.key_counts(keys[good], 6))
    moved = oracle.transform_points(q, np.eye(3), f64_points=not flags)
    want_hist, want_ov = R.match_keys(t, keys, moved, 0.5, 6)
    assert ov == want_ov and np.array_equal(hist, want_hist)
    hist, ov, ov2 = _match_case(ctx, flags, t, keys, q[bad], 6)     # nothing but broken sources
    assert ov == ov2 == 0 and not hist.any()


@DTYPES
def test_match_keys_many_with_jobs_whose_blocks_return_early_and_keys_beyond_the_histogram(ctx, flags):
    """sources of 1, 600 and 0 points in one launch: three blocks per job, of which the first job uses one and the last none"""
    s = st.CloudStore(ctx, capacity_points=1 << 14, max_clouds=16)
    targets = [R.lattice(2049), R.lattice(700, origin=(-300.0, 8.0)), R.lattice(100)]
    keys = [(np.arange(len(t)) % 10).astype(np.int32) for t in targets]
    far = np.where(np.arange(600) % 7 == 3, np.float32(2.0), np.float32(0.0))[:, None]
    sources = [targets[0][[2048]] + R.OFFSETS[1], targets[1][:600] + R.OFFSETS[np.arange(600) % 5] + far,
               np.zeros((0, 2), np.float32)]
    ht = [s.put_keys(t, k) for t, k in zip(targets, keys)]
    hq = [s.put(q) for q in sources]
    for n_keys in (4, 0):
        hists, ovs = s.match_keys_many(hq, [EYE6] * 3, ht, 0.5, n_keys, flags=flags)
        assert hists.shape == (3, n_keys)
        for t, k, q, hist, ov in zip(targets, keys, sources, hists, ovs):
            want_hist, want_ov = R.match_keys(t, k, q, 0.5, n_keys)
            assert ov == want_ov and np.array_equal(hist, want_hist)
        assert ovs.tolist() == [1, 600 - 86, 0]
        if n_keys:
            assert hists[0].tolist() == [0, 0, 0, 0] and 0 < hists[1].sum() < ovs[1]     # key 8 of target 2048: overlap only
    s.close()


def test_overlap_with_an_unused_handle_on_either_side_is_zero(ctx):
    rng = np.random.default_rng(43)
    s = st.CloudStore(ctx, capacity_points=1 << 12, max_clouds=8)
    a = s.put(_cloud(rng, 300))
    assert s.overlap([(a, a), (-1, a), (a, -1), (-1, -1)], [EYE6] * 4, 0.5).tolist() == [300, 0, 0, 0]
    s.close()


# ---- compact_selected(_many) --------------------------------------------------------------------------------------------------
COMPACT_SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 3000)
SELECTIONS = {
    "none": lambda n, rng: np.zeros(n, bool),
    "all": lambda n, rng: np.ones(n, bool),
    "last": lambda n, rng: np.arange(n) == n - 1,
    "lane_63": lambda n, rng: np.arange(n) % 64 == 63,
    "chunk_start": lambda n, rng: np.arange(n) % 1024 == 0,
    "random": lambda n, rng: rng.random(n) < 0.5,
}


def _keyed_cloud(rng, n):
    return _cloud(rng, n), rng.integers(0, 1000, n).astype(np.int32)


@pytest.mark.parametrize("kind", list(SELECTIONS))
def test_compact_selected_at_wave_and_chunk_edges(ctx, kind):
    rng = np.random.default_rng(51)
    s = st.CloudStore(ctx, capacity_points=1 << 16, max_clouds=128)
    for n in COMPACT_SIZES:
        (gp0, gk0), (pts, keys), (gp1, gk1) = _keyed_cloud(rng, 70), _keyed_cloud(rng, n), _keyed_cloud(rng, 70)
        g0, h, g1 = s.put_keys(gp0, gk0), s.put_keys(pts, keys), s.put_keys(gp1, gk1)
        sel = SELECTIONS[kind](n, rng)
        s.set_selection(h, sel)
        c = s.compact_selected(h, stamp=n)
        want_p, want_k = R.compact(pts, keys, sel)
        assert s.counts([c])[0] == int(sel.sum()) and s.meta(c, 1)[0].tolist() == [n]
        assert np.array_equal(s.read(c), want_p) and np.array_equal(s.read_keys(c), want_k), n
        for hh, p, k in ((g0, gp0, gk0), (h, pts, keys), (g1, gp1, gk1)):     # the source and its neighbours in the pool
            assert np.array_equal(s.read(hh), p) and np.array_equal(s.read_keys(hh), k), n
    s.close()


def test_compact_selected_many_with_an_empty_cloud_and_an_empty_selection(ctx):
    rng = np.random.default_rng(52)
    s = st.CloudStore(ctx, capacity_points=1 << 14, max_clouds=16)
    clouds = [_keyed_cloud(rng, n) for n in (3000, 0, 1025, 64)]
    sels = [SELECTIONS[kind](len(p), rng) for kind, (p, _) in zip(("random", "all", "last", "none"), clouds)]
    hs = [s.put_keys(p, k) for p, k in clouds]
    for h, sel in zip(hs, sels):
        s.set_selection(h, sel)
    out = s.compact_selected_many(hs, stamps=[5, 6, 7, 8])
    assert out.tolist() == [4, 5, 6, 7] and s.counts(out).tolist() == [int(sels[0].sum()), 0, 1, 0]
    for c, (p, k), sel in zip(out, clouds, sels):
        want_p, want_k = R.compact(p, k, sel)
        assert np.array_equal(s.read(c), want_p) and np.array_equal(s.read_keys(c), want_k)
    for h, (p, k) in zip(hs, clouds):
        assert np.array_equal(s.read(h), p) and np.array_equal(s.read_keys(h), k)
    s.close()


# ---- fov_select(_many) --------------------------------------------------------------------------------------------------------
def test_fov_select_many_with_jobs_of_no_one_and_three_frames(ctx):
    jobs = R.fov_inputs()
    s = st.CloudStore(ctx, capacity_points=1 << 13, max_clouds=32)
    hs = [s.put_keys(pts, keys) for pts, keys, _, _, _ in jobs]
    hist, n_sel, n_amb = s.fov_select_many(hs, [[st.pose_T6(f) for f in j[2]] for j in jobs], [j[3] for j in jobs],
                                           [j[4] for j in jobs], R.FOV_N_KEYS)
    out = s.compact_selected_many(hs)
    assert n_amb.tolist() == [0] * len(jobs) and hist.shape == (len(jobs), R.FOV_N_KEYS)
    beyond = 0
    for j, (pts, keys, frames, rb, bb) in enumerate(jobs):
        assert not R.fov_near_a_bound(pts, frames, bb).any()
        sel = FrontEnd._fov_numpy(pts, frames, rb, bb)
        assert n_sel[j] == int(sel.sum()) and np.array_equal(hist[j], R.key_counts(keys[sel], R.FOV_N_KEYS)), j
        assert np.array_equal(s.read(out[j]), pts[sel]) and np.array_equal(s.read_keys(out[j]), keys[sel]), j
        beyond += int(n_sel[j] > hist[j].sum())                # selected points whose key has no bin: counted, not binned
        # ... and the same job on its own
        hist1, n_sel1, n_amb1 = s.fov_select(hs[j], [st.pose_T6(f) for f in frames], rb, bb, R.FOV_N_KEYS)
        assert n_sel1 == n_sel[j] and n_amb1 == 0 and np.array_equal(hist1, hist[j])
    assert beyond >= 3
    # the job without frames selected nothing, and its selection is a valid one: an empty keyed cloud comes out of it
    k = R.FOV_FRAMES_PER_JOB.index(0)
    assert n_sel[k] == 0 and not hist[k].any() and len(jobs[k][0]) == 256
    c = s.compact_selected(hs[k])
    assert s.read(c).shape == (0, 2) and s.read_keys(c).shape == (0,)
    s.close()


def test_fov_range_bound_is_exact(ctx):
    s = st.CloudStore(ctx, capacity_points=1 << 10, max_clouds=16)
    pts, keys = np.float32([[3, 4], [-3, 4], [4, -3], [0, 5]]), np.int32([0, 1, 2, 3])     # all at range exactly 5
    h = s.put_keys(pts, keys)
    eye = [st.pose_T6(Pose2(0.0, 0.0, 0.0))]
    above = np.nextafter(5.0, 6.0)
    for rb, bb, want in ((5.0, 3.0, [0, 0, 0, 0]), (above, 3.0, [1, 1, 1, 1]), (above, 1.0, [1, 0, 1, 0])):
        assert FrontEnd._fov_numpy(pts, [Pose2(0.0, 0.0, 0.0)], [rb], [bb]).tolist() == [bool(w) for w in want]
        hist, n_sel, n_amb = s.fov_select(h, eye, [rb], [bb], 4)
        assert hist.tolist() == want and n_sel == sum(want) and n_amb == 0, (rb, bb)
        c = s.compact_selected(h)
        assert np.array_equal(s.read(c), pts[np.array(want, bool)]) and np.array_equal(s.read_keys(c), keys[np.array(want, bool)])
    s.close()


# ---- concatenation and gather -------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("split", [(100, 155), (100, 156), (100, 157)], ids=["255", "256", "257"])
def test_get_points_keys_many_with_an_empty_job_first_and_gaps_behind_short_jobs(ctx, flags, split):
    rng = np.random.default_rng(61)
    s = st.CloudStore(ctx, capacity_points=1 << 15, max_clouds=64)
    sizes = (0, 0, split[0], split[1], 1, 1023, 1025, 700)
    clouds = [_cloud(rng, n) for n in sizes]
    hs = [s.put(c) for c in clouds]
    poses = [Pose2(*q) for q in rng.normal(0, [3, 3, 0.3], (len(clouds), 3))]
    jobs = [[0, 1], [0, 2, 1, 3, 0], [4], [5, 6, 7]]      # empty; zero-point clouds at the start, in the middle and at the end
    job_keys = [[3, 4], [5, 6, 7, 8, 9], [10], [11, 12, 13]]
    T6 = [[st.pose_T6(poses[k]) for k in job] for job in jobs]
    for res in (0.0, 0.5):
        base = len(s)
        out = s.get_points_keys_many([[hs[k] for k in job] for job in jobs], T6, job_keys, res, flags=flags, stamps=[1, 2, 3, 4])
        assert out.tolist() == list(range(base, base + len(jobs)))
        for job, ks, h in zip(jobs, job_keys, out):
            allp = np.concatenate([oracle.transform_points(clouds[k], poses[k].matrix(), f64_points=not flags) for k in job])
            allk = np.concatenate([np.full(len(clouds[k]), key, np.int32) for k, key in zip(job, ks)])
            if res > 0 and len(allp):
                allp, idx = oracle.downsample(allp, res, return_index=True)
                allk = allk[idx]
            assert np.array_equal(s.read(h), allp) and np.array_equal(s.read_keys(h), allk), (job, res)
        assert s.counts(out)[[0, 2]].tolist() == [0, 1] and (res > 0 or s.counts(out)[1] == sum(split))
        s.truncate(base)
    for h, c in zip(hs, clouds):
        assert np.array_equal(s.read(h), c)
    s.close()


@DTYPES
def test_get_points_with_clouds_around_the_gather_stride_and_unused_handles_between(ctx, flags):
    rng = np.random.default_rng(62)
    s = st.CloudStore(ctx, capacity_points=1 << 14, max_clouds=64)
    clouds = [_cloud(rng, n) for n in (1023, 1025, 1)]
    hs = [s.put(c) for c in clouds]
    poses = [Pose2(*q) for q in rng.normal(0, [3, 3, 0.3], (3, 3))]
    jobs = [[0, -1, 1, -1, 2], [2, -1, -1, 0, -1], [-1, -1, 1, -1, -1], [2, -1, -1, -1, -1]]
    handles = np.array([[hs[k] if k >= 0 else -1 for k in job] for job in jobs], np.int32)
    T6 = np.array([[st.pose_T6(poses[max(k, 0)]) for k in job] for job in jobs], np.float32)
    for res in (0.5, 0.0):
        base = len(s)
        out = s.get_points(handles, T6, res, flags=flags)
        for job, h in zip(jobs, out):
            ks = [k for k in job if k >= 0]
            if res > 0:
                want = oracle.get_points([clouds[k] for k in ks], [poses[k].matrix() for k in ks], res, f64_points=not flags)
            else:
                want = np.concatenate([oracle.transform_points(clouds[k], poses[k].matrix(), f64_points=not flags) for k in ks])
            assert np.array_equal(s.read(h), want), (job, res)
        s.truncate(base)
    s.close()


# ---- bbox ---------------------------------------------------------------------------------------------------------------------
def test_bbox_with_every_extreme_at_the_first_and_at_the_last_index(ctx):
    rng = np.random.default_rng(71)
    s = st.CloudStore(ctx, capacity_points=1 << 12, max_clouds=16)
    clouds = []
    for k, n in enumerate((1, 63, 64, 65, 255, 256, 257, 1025)):
        p = rng.uniform(-50, 50, (n, 2)).astype(np.float32)
        a, b = (0, n - 1) if k % 2 == 0 else (n - 1, 0)
        p[a] = (-100 - k, 100 + k)            # min x and max y
        if n > 1:
            p[b] = (100 + k, -100 - k)        # max x and min y
        clouds.append(p)
    hs = [s.put(c) for c in clouds]
    got = s.bbox(hs[::-1])
    assert got.dtype == np.float32 and np.array_equal(got, np.stack([R.bbox(c) for c in clouds[::-1]]))
    assert np.array_equal(got[-1], np.float32([-100, 100, -100, 100]))        # the cloud of one point
    assert np.array_equal(got[0], np.float32([-107, -107, 107, 107]))
    s.close()


def test_bbox_of_an_empty_cloud_and_of_clouds_that_are_not_there(ctx):
    """an empty cloud has the box the reduction starts from; matching_cost._StoreGrids, the one caller, refuses a box that is not
    finite with an error that names the cloud"""
    rng = np.random.default_rng(72)
    s = st.CloudStore(ctx, capacity_points=100, max_clouds=8)
    a, e = s.put(_cloud(rng, 50)), s.put(np.zeros((0, 2), np.float32))
    full = s.put(_cloud(rng, 80))
    assert s.counts([full])[0] == R.OVERFLOW
    inf = np.float32(np.inf)
    assert np.array_equal(s.bbox([e, a])[0], np.float32([inf, inf, -inf, -inf]))
    for bad in (full, len(s), -1):
        with pytest.raises(_lib.SonarFEError):
            s.bbox([a, bad])
    assert np.array_equal(s.bbox([a])[0], R.bbox(s.read(a)))                 # the store is usable after the refusals
    s.close()
