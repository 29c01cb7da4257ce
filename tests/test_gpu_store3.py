"""GPU: the keyframe store for N x 3 clouds (sfe_store3.hip, ``store.CloudStore3``).  Every comparison is bit for bit
(``np.array_equal``): the device code is deterministic and the references (tests/store3_ref.py: the reference's numpy transform,
np.concatenate, the 3-D downsample restatement of tests/pcl3_ref.py, a brute-force overlap count) are exact restatements, so
there are no tolerances.  ``get_points`` and ``overlap`` are also held to the host-pointer ``pcl`` calls on host-built inputs,
``icp`` to ``pcl.ICP.compute_jobs`` on the same host arrays (clouds and parameters from tests/icp3_cases.py).

Shapes (the kernels: 256 threads per workgroup and one point per lane, one-workgroup stages of 1024 threads, LDS tiles of 2048
points, the ICP kernel's 1024 queries per pass and 4096 resident targets): clouds of 0, 1, 255, 256, 257, 2049 points; job
totals 1023 .. 2049; 1, 2 and 33 jobs of 1 .. 5048 points; overlap sources 1 .. 257 on targets 2047 .. 4097."""
import numpy as np
import pytest

from sonar_slam_amd import _lib as L
from sonar_slam_amd import pcl
from sonar_slam_amd.store import CloudStore3

import icp3_cases as C
import store3_ref as R

pytestmark = pytest.mark.gpu
f32 = np.float32


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _state(s):
    st, off, cnt = s.meta()
    return len(s), st.tolist(), off.tolist(), cnt.tolist()


def _compact(s):
    _, off, cnt = s.meta()
    assert off[0] == 0 if len(off) else True
    assert np.array_equal(off[1:], (off + cnt)[:-1])


# ---- put, read, meta ------------------------------------------------------------------------------------------------------------
def test_put_read_meta(ctx):
    s = CloudStore3(ctx, capacity_points=4096, max_clouds=16)
    clouds = [R.cloud(10 + n, n) for n in R.PUT_SIZES]
    handles = [s.put(c, stamp=100 + k) for k, c in enumerate(clouds)]
    assert handles == list(range(len(clouds))) and len(s) == len(clouds)
    st, off, cnt = s.meta()
    assert st.tolist() == [100 + k for k in range(len(clouds))]
    assert cnt.tolist() == list(R.PUT_SIZES)
    assert off.tolist() == np.r_[0, np.cumsum(R.PUT_SIZES)[:-1]].tolist()
    assert s.counts([5, 0, 2]).tolist() == [2049, 0, 255]
    for h, c in zip(handles, clouds):
        got = s.read(h)
        assert got.shape == (len(c), 3) and _same(got, c)
    # after truncate the next put reuses the handle and the pool
    s.truncate(3)
    assert len(s) == 3
    c = R.cloud(77, 300)
    assert s.put(c, stamp=5) == 3
    assert s.meta(3, 1)[1][0] == 1 + 255 and _same(s.read(3), c)
    assert _same(s.read(2), clouds[2])
    s.truncate(0)
    assert len(s) == 0 and s.put(clouds[1]) == 0
    s.close()


def test_put_overflow_changes_nothing(ctx):
    s = CloudStore3(ctx, capacity_points=1000, max_clouds=3)
    a, b, c = R.cloud(1, 600), R.cloud(2, 600), R.cloud(3, 400)
    assert s.put(a, stamp=1) == 0
    before = _state(s)
    with pytest.raises(L.SonarFEError, match="error -4"):     # SFE_ERR_CAP
        s.put(b, stamp=2)
    assert _state(s) == before and len(s) == 1
    assert s.put(c, stamp=3) == 1                             # the next handle is unchanged; exact fill
    assert _same(s.read(0), a) and _same(s.read(1), c)
    assert s.put(np.zeros((0, 3), f32)) == 2
    before = _state(s)
    with pytest.raises(L.SonarFEError, match="error -4"):     # the slot table is full
        s.put(np.zeros((0, 3), f32))
    assert _state(s) == before
    s.close()


# ---- get_points -----------------------------------------------------------------------------------------------------------------
def _held(s, handle, clouds, Hs, resolution, ctx):
    """the stored result against store3_ref and against pcl.downsample on the host-built concatenation"""
    got = s.read(handle)
    want = R.get_points(clouds, Hs, resolution)
    print("get_points", [len(c) for c in clouds], "resolution", resolution, "->", len(got), "reference", len(want))
    assert _same(got, want)
    cat = R.concat(clouds, Hs)
    if resolution > 0 and len(cat):
        assert _same(got, pcl.downsample(cat, resolution, ctx=ctx))


def test_get_points_identity_without_downsample_returns_the_cloud(ctx):
    s = CloudStore3(ctx, capacity_points=8192, max_clouds=16)
    c = R.cloud(31, 777)
    h = s.put(c)
    for res in (0.0, -1.0):
        out = s.get_points([[h]], [[R.EYE]], res, stamps=[42])
        assert _same(s.read(out[0]), c)
    assert s.meta()[0].tolist() == [0, 42, 42]
    _compact(s)
    s.close()


def test_get_points_unused_and_empty_inputs(ctx):
    s = CloudStore3(ctx, capacity_points=1 << 14, max_clouds=32)
    a, b, e = R.cloud(41, 700), R.cloud(42, 300), np.zeros((0, 3), f32)
    ha, hb, he = s.put(a), s.put(b), s.put(e)
    Hs = [R.motion(43), R.motion(44), R.motion(45)]
    out = s.get_points([[ha, -1, hb], [ha, he, hb], [-1, -1, -1], [he], [-1, hb]],
                       [Hs, Hs, Hs, Hs[:1], Hs[:2]], 2.0)
    assert out.tolist() == [3, 4, 5, 6, 7]
    _held(s, out[0], [a, b], [Hs[0], Hs[2]], 2.0, ctx)
    _held(s, out[1], [a, b], [Hs[0], Hs[2]], 2.0, ctx)
    assert s.counts(out).tolist()[2:4] == [0, 0]              # only -1, and only an empty cloud: empty slots
    assert s.read(out[2]).shape == (0, 3)
    _held(s, out[4], [b], [Hs[1]], 2.0, ctx)
    _compact(s)
    s.close()


@pytest.mark.parametrize("total", R.TOTALS)
def test_get_points_job_totals_at_the_tile_edges(ctx, total):
    s = CloudStore3(ctx, capacity_points=1 << 14, max_clouds=16)
    clouds, Hs = R.total_job(total)
    hs = [s.put(c) for c in clouds]
    for res in (16.0, 0.0):
        out = s.get_points([hs], [Hs], res)
        _held(s, out[0], clouds, Hs, res, ctx)
    assert s.counts([4])[0] == total
    _compact(s)
    s.close()


@pytest.mark.parametrize("n_jobs", [1, 2, 33])
def test_get_points_many_jobs_of_mixed_sizes(ctx, n_jobs):
    clouds, jobs = R.mixed_jobs(n_jobs)
    s = CloudStore3(ctx, capacity_points=1 << 19, max_clouds=64)
    hs = [s.put(c) for c in clouds]
    out = s.get_points([[hs[i] if i >= 0 else -1 for i in ids] for ids, _ in jobs], [Hs for _, Hs in jobs], 16.0,
                       stamps=np.arange(n_jobs) + 7)
    assert out.tolist() == list(range(len(clouds), len(clouds) + n_jobs))
    assert s.meta(len(clouds))[0].tolist() == list(range(7, 7 + n_jobs))
    for (ids, Hs), h in zip(jobs, out):
        used = [(clouds[i], H) for i, H in zip(ids, Hs) if i >= 0]
        _held(s, h, [c for c, _ in used], [H for _, H in used], 16.0, ctx)
    _compact(s)
    s.close()


def test_get_points_resolutions_one_leaf_per_point_and_one_leaf_for_all(ctx):
    s = CloudStore3(ctx, capacity_points=1 << 13, max_clouds=16)
    a, b = R.cloud(51, 900), R.cloud(52, 400)
    ha, hb = s.put(a), s.put(b)
    Hs = [R.motion(53), R.motion(54)]
    fine, coarse = s.get_points([[ha, hb]], [Hs], 1e-4)[0], s.get_points([[ha, hb]], [Hs], 1e4)[0]
    assert s.counts([fine, coarse]).tolist() == [1300, 1]
    _held(s, fine, [a, b], Hs, 1e-4, ctx)
    _held(s, coarse, [a, b], Hs, 1e4, ctx)
    # a resolution that the boundary's rounding (std::to_string and back) changes: as pcl.downsample rounds it
    odd = s.get_points([[ha, hb]], [Hs], 2.00000049)[0]
    _held(s, odd, [a, b], Hs, 2.00000049, ctx)
    s.close()


def test_get_points_output_feeds_the_next_call_and_placement_is_compact(ctx):
    s = CloudStore3(ctx, capacity_points=1 << 14, max_clouds=16)
    a, b = R.cloud(61, 1500), R.cloud(62, 1100)
    ha, hb = s.put(a), s.put(b)
    H1, H2, H3 = R.motion(63), R.motion(64), R.motion(65, big=False)
    t1 = s.get_points([[ha, hb]], [[H1, H2]], 5.0)[0]
    first = s.read(t1)
    assert _same(R.transform(first, H3), R.transform_fma(first, H3))   # (a device result moved: not among R.fixed_inputs)
    t2 =s.get_points([[t1, ha]], [[H3, R.EYE]], 2.5)[0]
    _held(s, t2, [first, a], [H3, R.EYE], 2.5, ctx)
    _, off, cnt = s.meta()
    assert cnt[t1] < 2600 and off[t2] == off[t1] + cnt[t1]    # right behind the downsampled cloud, not behind the bound
    nxt = s.put(b)
    assert s.meta(nxt, 1)[1][0] == off[t2] + cnt[t2]
    _compact(s)
    s.close()


def test_get_points_overflow_changes_nothing(ctx):
    s = CloudStore3(ctx, capacity_points=2000, max_clouds=4)
    a, b = R.cloud(71, 700), R.cloud(72, 500)
    ha, hb = s.put(a), s.put(b)
    before = _state(s)
    # the upper bound (1200) does not fit the 800 points left, though the downsampled cloud would
    with pytest.raises(L.SonarFEError, match="error -4"):
        s.get_points([[ha, hb]], [[R.EYE, R.EYE]], 1e4)
    assert _state(s) == before
    # the pool has room for each, the slot table has not: 3 jobs, 2 slots
    with pytest.raises(L.SonarFEError, match="error -4"):
        s.get_points([[hb], [-1], [-1]], [[R.EYE], [R.EYE], [R.EYE]], 1e4)
    assert _state(s) == before
    with pytest.raises(L.SonarFEError, match="error -1"):     # an unknown handle
        s.get_points([[2]], [[R.EYE]], 1.0)
    assert _state(s) == before
    out = s.get_points([[ha]], [[R.EYE]], 1e4)
    assert out.tolist() == [2] and s.counts(out).tolist() == [1]
    assert _same(s.read(0), a) and _same(s.read(1), b)
    s.close()


# ---- icp ------------------------------------------------------------------------------------------------------------------------
def _host_icp(ctx, p, srcs, tgts, guesses):
    """pcl.ICP.compute_jobs on host arrays: one job per (source, target, guess)"""
    icp = pcl.ICP(ctx=ctx)
    icp.setParams(p)
    so, to = np.r_[0, np.cumsum([len(x) for x in srcs])], np.r_[0, np.cumsum([len(x) for x in tgts])]
    jobs4 = np.array([[so[k], len(srcs[k]), to[k], len(tgts[k])] for k in range(len(srcs))], np.int32)
    g = np.stack(guesses).astype(f32).reshape(len(srcs), 16)
    return icp.compute_jobs(np.concatenate(srcs), np.concatenate(tgts), jobs4, g)


@pytest.mark.parametrize("name", ["ns1025", "nt4097", "ties", "max_dist_drops_all", "no_finite_distance"])
def test_icp_equals_the_host_pointer_call(ctx, name):
    src, tgt, g, p = C.job(name)
    s = CloudStore3(ctx, capacity_points=1 << 14, max_clouds=8)
    s.put(R.cloud(1, 37))                                     # the clouds do not begin at the pool's start
    hs, ht = s.put(src), s.put(tgt)
    st, T, it = s.icp([[hs, ht]], [g], p)
    want = _host_icp(ctx, p, [src], [tgt], [g])
    print(name, "status", st, want[0], "iterations", it, want[2])
    assert _same(st, want[0]) and _same(T, want[1]) and _same(it, want[2])
    assert T.shape == (1, 4, 4) and T.dtype == np.float32
    if name in ("max_dist_drops_all", "no_finite_distance"):
        assert int(st[0]) in (1, 2) and _same(T[0], g)        # a failure: T is the guess
    else:
        assert int(st[0]) == 0
    s.close()


def test_icp_mixed_launch_sharing_clouds_and_a_self_pair(ctx):
    srcs, tgts, jobs, p = C.mixed_launch()
    s = CloudStore3(ctx, capacity_points=1 << 16, max_clouds=32)
    hs, ht = [s.put(c) for c in srcs], [s.put(c) for c in tgts]
    pairs = [[hs[a], ht[b]] for a, b, _ in jobs]
    st, T, it = s.icp(pairs, [g for _, _, g in jobs], p)
    want = _host_icp(ctx, p, [srcs[a] for a, _, _ in jobs], [tgts[b] for _, b, _ in jobs], [g for _, _, g in jobs])
    print("mixed", st, it)
    assert _same(st, want[0]) and _same(T, want[1]) and _same(it, want[2])
    assert st.tolist() == [0, 0, 2, 0, 0, 0, 0, 0]
    # source and target the same handle
    g = np.asarray(C.rigid((0.2, 0.7, -0.4), 0.02, (0.03, 0.02, -0.01)), f32)
    st, T, it = s.icp([[ht[0], ht[0]]], [g], p)
    want = _host_icp(ctx, p, [tgts[0]], [tgts[0]], [g])
    assert _same(st, want[0]) and _same(T, want[1]) and _same(it, want[2]) and int(st[0]) == 0
    s.close()


def test_icp_refuses_empty_and_unknown_clouds(ctx):
    src, tgt, g, p = C.job("ns1")
    s = CloudStore3(ctx, capacity_points=4096, max_clouds=8)
    hs, ht, he = s.put(src), s.put(tgt), s.put(np.zeros((0, 3), f32))
    for pair in ([hs, he], [he, ht], [hs, 3], [3, ht], [-1, ht]):
        T = None
        with pytest.raises(L.SonarFEError, match="error -1"):     # SFE_ERR_ARG, before any launch
            T = s.icp([[hs, ht], pair], [g, g], p)
        assert T is None
    st, T, it = s.icp([[hs, ht]], [g], p)
    assert _same(T, _host_icp(ctx, p, [src], [tgt], [g])[1])
    s.close()


# ---- overlap --------------------------------------------------------------------------------------------------------------------
def _host_overlap(ctx, src, H, tgt, max_dist):
    ids, _ = pcl.match(tgt, R.transform(src, H), 1, max_dist, ctx=ctx)
    return int((ids[0] != -1).sum())


@pytest.mark.parametrize("nt", R.OVL_TARGETS)
def test_overlap_source_and_target_sizes(ctx, nt):
    s = CloudStore3(ctx, capacity_points=1 << 15, max_clouds=16)
    pairs, Hs, want = [], [], []
    for ns in R.OVL_SOURCES:
        src, H, tgt, r = R.overlap_pair(ns, nt)
        pairs.append([s.put(src), s.put(tgt)])
        Hs.append(H)
        want.append(R.overlap(src, H, tgt, r))
        assert want[-1] == _host_overlap(ctx, src, H, tgt, r)
    one = [int(s.overlap([p], [H], 0.3)[0]) for p, H in zip(pairs, Hs)]          # 1 job per call
    print("overlap nt", nt, "counts", one, "reference", want)
    assert one == want and 0 < sum(want) < sum(R.OVL_SOURCES)
    assert s.overlap(pairs, Hs, 0.3).tolist() == want
    s.close()


def test_overlap_boundaries_nan_and_infinite_points(ctx):
    src, tgt, max_dist, expected = R.boundary_case()
    s = CloudStore3(ctx, capacity_points=4096, max_clouds=8)
    hs, ht, he = s.put(src), s.put(tgt), s.put(np.zeros((0, 3), f32))
    assert R.overlap(src, R.EYE, tgt, max_dist) == expected == _host_overlap(ctx, src, R.EYE, tgt, max_dist)
    assert s.overlap([[hs, ht]], [R.EYE], max_dist).tolist() == [expected]
    # one at a time: exactly at the bound counts, the next float beyond it does not, NaN and infinities never
    singles = [s.put(src[k:k + 1]) for k in range(5)]
    assert s.overlap([[h, ht] for h in singles], [R.EYE] * 5, max_dist).tolist() == [1, 0, 0, 0, 0]
    assert s.overlap([[hs, he], [he, ht], [hs, ht]], [R.EYE] * 3, max_dist).tolist() == [0, 0, expected]
    assert s.overlap([[hs, ht]], [R.EYE], np.inf).tolist() == [_host_overlap(ctx, src, R.EYE, tgt, np.inf)]
    with pytest.raises(L.SonarFEError, match="error -1"):
        s.overlap([[hs, 99]], [R.EYE], max_dist)
    s.close()


def test_overlap_forty_jobs_of_mixed_sizes(ctx):
    s = CloudStore3(ctx, capacity_points=1 << 16, max_clouds=64)
    clouds, pairs, Hs = R.forty_jobs()
    hs = [s.put(c) for c in clouds]
    want = [R.overlap(clouds[a], H, clouds[b], 0.5) for (a, b), H in zip(pairs, Hs)]
    got = s.overlap([[hs[a], hs[b]] for a, b in pairs], Hs, 0.5).tolist()
    print("overlap 40 jobs", got)
    assert got == want and sum(1 for w in want if w > 0) >= 5
    s.close()


# ---- a small session ------------------------------------------------------------------------------------------------------------
def test_small_session_equals_the_host_pointer_calls(ctx):
    """six keyframes of about 300 points; each step: a target from the last three keyframes, a scan match, an overlap"""
    p = C.params()
    frames, _ = R.session()
    s = CloudStore3(ctx, capacity_points=1 << 14, max_clouds=32)
    hk = [s.put(c, stamp=k) for k, c in enumerate(frames)]
    icp = pcl.ICP(ctx=ctx)
    icp.setParams(p)
    for k in range(3, 6):
        _, between, guess = R.session_step(k)
        base = len(s)
        # over handles
        tgt_h = int(s.get_points([hk[k - 3:k]], [between], 0.1)[0])
        st, T, it = s.icp([[hk[k], tgt_h]], [guess], p)
        ov = s.overlap([[hk[k], tgt_h]], [T[0]], 0.2)
        target = s.read(tgt_h)
        s.truncate(base)                                      # the step's target is dropped, as chained does in 2-D
        assert len(s) == 6
        # the same step through the host-pointer calls
        cat = np.concatenate([R.transform(frames[i], H) for i, H in zip((k - 3, k - 2, k - 1), between)])
        target_h = pcl.downsample(cat, 0.1, ctx=ctx)
        st_h, T_h, it_h = icp.compute_jobs(frames[k], target_h, np.array([[0, len(frames[k]), 0, len(target_h)]], np.int32),
                                           guess.reshape(1, 16))
        moved = R.transform(frames[k], T_h[0])
        assert _same(moved, R.transform_fma(frames[k], T_h[0]))   # (a pose the device found: not among R.fixed_inputs)
        ids, _ = pcl.match(target_h, moved, 1, 0.2, ctx=ctx)
        print("step", k, "target", len(target), "status", st, "iterations", it, "overlap", ov)
        assert _same(target, target_h)
        assert _same(st, st_h) and _same(T, T_h) and _same(it, it_h) and int(st[0]) == 0
        assert int(ov[0]) == int((ids[0] != -1).sum()) and 0 < int(ov[0]) <= len(frames[k])
    s.close()
