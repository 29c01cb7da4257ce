"""The SLAM cloud (slam_ros.py:317-359, publish_point_cloud) built in the keyframe store, and its method-2 map rendered from
there: replay.FrontEnd.slam_cloud / occupancy_grid2 and chained.SessionBatch.slam_clouds / occupancy_grids2."""
import copy
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import oracle  # noqa: E402
from test_gpu_map_batch import _same_records  # noqa: E402
from test_gpu_mapping2 import info_of  # noqa: E402
from sonar_slam_amd.replay import CloudRef, FrontEnd, Keyframe  # noqa: E402
from sonar_slam_amd.store import CloudStore  # noqa: E402

pytestmark = pytest.mark.gpu

K, ROWS, N = 4, 256, 3
SETTINGS = dict(x0=0.0, y0=-20.0, width=40.0, height=40.0, inc=25.0, pub_occupancy2=True)


def same(a, b, tag=None):
    assert info_of(a) == info_of(b), tag
    assert a.occ.dtype == np.int8 and a.occ.shape == b.occ.shape and np.array_equal(a.occ, b.occ), tag
    assert a.data == b.data, tag


@pytest.fixture(scope="module")
def sessions():
    from test_global_init import _session
    from sonar_slam_amd.feature_extraction import SonarPing, oculus_bearings
    sess = [_session(K, rows=ROWS, step=1.7, turn=0.3, seed=21 + 4 * s, n_world=9000, start=(20.0 - 1.5 * s, 0.8 * s, 0.1 * s))
            for s in range(N)]
    frames, dr = np.stack([x[0] for x in sess]), np.stack([x[2] for x in sess])
    ping = SonarPing(frames[0][0], oculus_bearings(frames.shape[-1]), 30.0 / ROWS)
    return frames, dr, sess[0][4], ping


def front_end(ctx, sessions, s, feed="store"):
    from test_global_init import _replay_session
    frames, dr, bearings, ping = sessions
    store = CloudStore(ctx, capacity_points=1 << 18, max_clouds=64)
    front, log = _replay_session(ctx, frames[s], bearings, dr[s], ROWS, store, ssm_min_points=20, ssm_initialization=False,
                                 mapping=dict(ping=ping, feed=feed, **SETTINGS))
    assert len(log) == K and len(store) == K and len(front.keyframes) == K
    return front, log, store


def test_front_end_slam_cloud_and_its_map(ctx, sessions):
    front, log, store = front_end(ctx, sessions, 0)
    grid, records = front.map.logodds_grid.copy(), copy.deepcopy(log)
    ref = front.slam_cloud()
    assert isinstance(ref, CloudRef) and ref.handle == K and len(store) == K + 1
    points, keys = store.read(ref.handle), store.read_keys(ref.handle)
    assert len(points) == len(ref) == len(keys) > 200 and sorted(set(keys)) == list(range(K))
    store.truncate(ref.handle)
    # the host route of the same front end's clouds: FrontEnd.get_points_keys' numpy branch (pcl.downsample with keys)
    host = FrontEnd(ctx, point_resolution=front.point_resolution, nssm_enable=False)
    for kf in front.keyframes:
        copy_kf = Keyframe(True, kf.time, kf.dr_pose, store.read(kf.points.handle).astype(np.float64))
        copy_kf.update(kf.pose)
        host.keyframes.append(copy_kf)
    want_points, want_keys = host.get_points_keys(range(K))
    assert np.array_equal(points, want_points) and np.array_equal(keys, np.asarray(want_keys).ravel())
    cloud = host.slam_cloud()
    assert cloud.dtype == np.float32 and cloud.shape == (len(points), 4)
    assert np.array_equal(cloud, np.c_[points, np.zeros(len(points)), keys].astype(np.float32))
    # ... and the oracle's downsample with indices, as oracle/chain.py uses it
    parts = [oracle.transform_points(kf.points, kf.pose.matrix(), f64_points=True) for kf in host.keyframes]
    allk = np.concatenate([np.full(len(p), f, np.float32) for f, p in enumerate(parts)])
    o_points, idx = oracle.downsample(np.concatenate(parts), front.point_resolution, return_index=True)
    assert np.array_equal(points, o_points) and np.array_equal(keys, allk[idx].astype(np.int32))
    # the map of that cloud
    for kw in (dict(), dict(frames=[2, 0, 2, 9]), dict(resolution=0.5)):
        n = len(store)
        got = front.occupancy_grid2(**kw)
        assert len(store) == n == K
        front.map.point_cloud = cloud
        same(got, front.map.get_occupancy_grid2(**kw), kw)
        assert set(np.unique(got.occ)) == {-1, 0, 100}
    assert np.array_equal(front.map.logodds_grid, grid) and len(front.keyframes) == K
    _same_records(front.log, records)
    # a failure inside the call gives the slot back too
    with pytest.raises(IndexError):
        front.occupancy_grid2(frames=[77])
    assert len(store) == K
    front.map.close()
    store.close()


def test_session_batch_maps_equal_the_front_ends(ctx, sessions, shipped_cfar):
    from test_global_init import _product_fe
    from sonar_slam_amd import chained, icp_config
    frames, dr, bearings, ping = sessions

    def batch():
        fe = _product_fe(ctx)
        fe.generate_map_xy(ping)
        sb = chained.SessionBatch(ctx, fe.geometry, shipped_cfar.params["SOCA"], "SOCA", 65, icp_config.shipped_params(), N, K, dr,
                                  ssm_min_points=20, mapping=dict(ping=ping, max_pixels=1 << 16, feed="store", **SETTINGS))
        for k in range(K):
            sb.upload_frames(k, frames[:, k])
        return sb

    quiet = batch()
    quiet_recs, quiet_loops = copy.deepcopy(quiet.run()), copy.deepcopy(quiet.loops)
    sb = batch()
    mid = None
    for k in range(K):
        sb.step(k)
        n = len(sb.store)
        grids = sb.occupancy_grids2()               # between the steps: the keyframes recorded so far
        assert len(sb.store) == n == N * (k + 1) and len(grids) == N
        if k == 1:
            mid = grids
    _same_records(copy.deepcopy(sb.records), quiet_recs)
    assert sb.loops == quiet_loops
    for va, vb in zip(sb.maps.maps, quiet.maps.maps):
        assert np.array_equal(va.logodds_grid.view(np.int32), vb.logodds_grid.view(np.int32))
    handles = sb.slam_clouds([2, 0])
    assert list(handles) == [N * K, N * K + 1]
    part = [(sb.store.read(h), sb.store.read_keys(h)) for h in handles]
    sb.store.truncate(N * K)
    fronts = [front_end(ctx, sessions, s) for s in range(N)]
    for s, (front, log, store) in enumerate(fronts):
        for k in range(K):
            assert tuple(sb.records[k]["pose"][s]) == log[k]["pose"], (s, k)
    for i, s in enumerate([2, 0]):                  # the clouds themselves
        front, _, store = fronts[s]
        ref = front.slam_cloud()
        assert np.array_equal(store.read(ref.handle), part[i][0]) and np.array_equal(store.read_keys(ref.handle), part[i][1])
        assert len(part[i][0]) > 200
        store.truncate(ref.handle)
    for kw in (dict(), dict(frames=[3, 1, 1], resolution=0.5)):
        n = len(sb.store)
        got = sb.occupancy_grids2(**kw)
        assert len(sb.store) == n
        some = sb.occupancy_grids2(sessions=[2, 0], **kw)
        for s, (front, _, _) in enumerate(fronts):
            same(got[s], front.occupancy_grid2(**kw), (s, kw))
        same(some[0], got[2], kw)
        same(some[1], got[0], kw)
        assert all(set(np.unique(g.occ)) == {-1, 0, 100} for g in got)
        if not kw:                                  # two keyframes gave another map than four
            assert mid[0].occ.shape != got[0].occ.shape or not np.array_equal(mid[0].occ, got[0].occ)
    for front, _, store in fronts:
        front.map.close()
        store.close()
    quiet.free()
    sb.free()


def test_what_is_missing_is_named(ctx, sessions, shipped_cfar):
    from test_global_init import _product_fe
    from sonar_slam_amd import chained, icp_config
    frames, dr, bearings, ping = sessions
    fe = _product_fe(ctx)
    fe.generate_map_xy(ping)
    args = (ctx, fe.geometry, shipped_cfar.params["SOCA"], "SOCA", 65, icp_config.shipped_params(), 1, 2, dr[:1, :2])
    sb = chained.SessionBatch(*args)
    with pytest.raises(RuntimeError, match="no maps"):
        sb.occupancy_grids2()
    sb.free()
    sb = chained.SessionBatch(*args, mapping=dict(ping=ping, max_pixels=1 << 16, **dict(SETTINGS, pub_occupancy2=False)))
    with pytest.raises(RuntimeError, match="pub_occupancy2=False"):
        sb.occupancy_grids2()
    sb.free()
