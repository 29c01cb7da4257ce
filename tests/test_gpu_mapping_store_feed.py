"""Mapping.add_keyframe_store and replay.FrontEnd(mapping=...): a single occupancy map fed from a CloudStore on the device is,
bit for bit, the map add_keyframe builds from store.read(handle) -- and the one-session MapBatch fed from the same handles."""
import copy
import json
import os
import sys

import ctypes as C
import numpy as np
import pytest
from scipy.special import logit

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]
import mapping_ref  # noqa: E402
from test_gpu_map_batch import _same_records, device_shape, same  # noqa: E402
from test_gpu_map_store_feed import _near, cloud  # noqa: E402
from test_gpu_mapping import configured, ref_map, state  # noqa: E402
from sonar_slam_amd import _lib  # noqa: E402
from sonar_slam_amd.mapping import MapBatch, Mapping  # noqa: E402
from sonar_slam_amd.pose2 import Pose2  # noqa: E402
from sonar_slam_amd.store import CloudStore  # noqa: E402

pytestmark = pytest.mark.gpu

FIX = os.path.join(HERE, "golden", "mapping_session.npz")
# six adds: key 3 is missed; the map of the fixture's settings covers [-10, 10] x [-10, 10] and grows by 6 m: the fan of key 2
# (10.24 m, looking down and to the left) leaves it on top (rows < 0) and on the left, that of key 5 on the left again
KEYS = [0, 1, 2, 4, 5, 6]
POSES = [(0.0, 0.0, 0.1), (2.5, -2.0, 0.4), (-4.0, -5.0, -2.4), (1.0, 3.0, 1.5), (-9.0, 2.0, 3.0), (3.0, 4.0, -0.7)]
# 1500 crosses a 256-thread block of the per-point kernels and a 1024-point chunk; 0 is a keyframe without a measurement; a
# cluster of 20 is emptied by the filter at min_points = 20, one of 21 stays
SIZES = [1500, 300, 0, 21, 1500, 20]


@pytest.fixture(scope="module")
def fix():
    return np.load(FIX)


@pytest.fixture(scope="module")
def pings(fix):
    geoms = json.loads(str(fix["geoms"]))       # A: 128 beams x 256 ranges (r_skip 5), B: 256 x 128 (r_skip 2, c_skip 2)
    return {g: mapping_ref.SessionPing(*geoms[g]) for g in ("A", "B")}


@pytest.fixture(scope="module")
def clouds():
    return [cloud(n, 40 + i) for i, n in enumerate(SIZES)]


def new_map(ctx, fix, **over):
    return configured(Mapping(ctx), fix, **over)


def bits(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))


def same_grid_msgs(a, b, tag):
    assert bits(a.occ, b.occ), tag
    ia, ib = a.info, b.info
    assert (ia.width, ia.height, ia.resolution, ia.origin.position.x, ia.origin.position.y) == \
        (ib.width, ib.height, ib.resolution, ib.origin.position.x, ib.origin.position.y), tag


def same_map(a, b, tag):
    """two Mappings that were given the same calls: every bit of the state and of what they publish"""
    assert bits(a.logodds_grid, b.logodds_grid), tag
    assert (a.x0, a.y0, a.rows, a.cols, a.width, a.height) == (b.x0, b.y0, b.rows, b.cols, b.width, b.height), tag
    assert (a.rmin, a.rmax, a.cmin, a.cmax) == (b.rmin, b.rmax, b.cmin, b.cmax), tag
    assert a._grow == b._grow and device_shape(a) == device_shape(b) == (a.rows, a.cols, a._grow[0], a._grow[1]), tag
    assert (a.oculus_image_size, a.oculus_r_skip, a.oculus_c_skip) == (b.oculus_image_size, b.oculus_r_skip, b.oculus_c_skip)
    assert len(a.keyframes) == len(b.keyframes), tag
    for k, (ka, kb) in enumerate(zip(a.keyframes, b.keyframes)):
        assert (ka is None) == (kb is None), (tag, k)
        if ka is None:
            continue
        assert (ka.k, ka.box, ka.base, ka._slot) == (kb.k, kb.box, kb.base, kb._slot), (tag, k)
        for name in ("r", "c", "l", "logodds"):
            assert bits(getattr(ka, name), getattr(kb, name)), (tag, k, name)
    live = [k for k, kf in enumerate(a.keyframes) if kf is not None]
    for frames, resolution in ((None, None), (None, 0.5), (live[::2] + [99], None), (live[1:], 0.6)):
        same_grid_msgs(a.get_occupancy_grid1(frames, resolution), b.get_occupancy_grid1(frames, resolution),
                       (tag, frames, resolution))
    assert state(a) == state(b), tag


def same_stages(a, b, tag):
    for x, y in zip(a.measure_stages(), b.measure_stages()):
        assert bits(x, y), tag


def snapshot(m):
    """everything a refused add must leave alone (the objects of the sonar settings by identity)"""
    return (state(m), device_shape(m), [id(kf) for kf in m.keyframes], sorted((k, id(v)) for k, v in vars(m.oculus).items()),
            m.oculus_image_size, m.oculus_r_skip, m.oculus_c_skip, m._geom, m._hit_key, sorted(m._geom_shape.items()),
            dict(m.feed_stats), m._cloud_ref, m._point_cloud)


@pytest.mark.parametrize("min_points", [20, 1])
@pytest.mark.parametrize("geom", ["A", "B"])
def test_store_fed_map_is_the_host_fed_map(ctx, fix, pings, clouds, min_points, geom):
    host, dev = (new_map(ctx, fix, outlier_filter_min_points=min_points) for _ in range(2))
    store = CloudStore(ctx, capacity_points=1 << 14, max_clouds=16)
    ping = pings[geom]
    assert (int(np.floor(0.2 / ping.range_resolution)), geom) in ((5, "A"), (2, "B"))
    for key, p, pts in zip(KEYS, POSES, clouds):
        h = store.put(pts)
        host.add_keyframe(key, Pose2(*p), ping, store.read(h))
        dev.add_keyframe_store(key, Pose2(*p), ping, store, h)
        same_stages(host, dev, "key %d" % key)
    assert (int(dev.oculus_r_skip), int(dev.oculus_c_skip)) == {"A": (5, 1), "B": (2, 2)}[geom]
    assert dev._grow[0] > 0 and dev._grow[1] > 0 and dev.keyframes[3] is None and len(dev.keyframes) == 7
    same_map(host, dev, "%s, min_points %d" % (geom, min_points))
    assert np.count_nonzero(dev.logodds_grid) > 500
    new = [Pose2(p[0] + 0.7, p[1] - 1.1, p[2] + 0.2) for p in POSES]
    for m in (host, dev):
        m.update_poses(KEYS, new)
    same_map(host, dev, "after update_poses")
    stats = dev.feed_stats
    print("undecided %d of %d points" % (stats["undecided"], stats["points"]))
    assert stats["calls"] == len(KEYS) and stats["points"] == sum(SIZES) > 1000
    assert stats["undecided"] <= 0.01 * stats["points"]
    assert host.feed_stats == {"points": 0, "undecided": 0, "calls": 0}
    dev.configure()
    assert dev.feed_stats == {"points": 0, "undecided": 0, "calls": 0}
    for m in (host, dev):
        m.close()
    store.close()


@pytest.mark.parametrize("min_points", [20, 1])
def test_store_fed_map_is_a_one_session_map_batch(ctx, fix, pings, clouds, min_points):
    settings = dict(json.loads(str(fix["settings"])), outlier_filter_min_points=min_points)
    m = new_map(ctx, fix, outlier_filter_min_points=min_points)
    b = MapBatch(ctx, 1, 8, max_pixels=8192, **settings)
    b.configure()
    store = CloudStore(ctx, capacity_points=1 << 14, max_clouds=16)
    for i, (key, p, pts) in enumerate(zip(KEYS, POSES, clouds)):
        ping = pings["AB"[i >= 3]]                                  # the geometry changes half way
        h = store.put(pts)
        m.add_keyframe_store(key, Pose2(*p), ping, store, h)
        b.add_keyframes_store([0], [key], [Pose2(*p)], ping, store, [h])
        for x, y in zip(m.measure_stages(), b.maps[0].measure_stages()):
            assert bits(x, y), key
    same(b.maps[0], m, "min_points %d" % min_points)
    assert m.feed_stats == b.feed_stats and m.feed_stats["points"] == sum(SIZES)
    m.close()
    b.close()
    store.close()


@pytest.mark.parametrize("min_points", [8, 1])
def test_undecided_points_take_the_host_route(ctx, fix, pings, min_points):
    """the origin, points on a rounding boundary of the bearing column (within 1e-7 columns of x.5) and on both ends of the
    bearing table (within a float32 ulp): the device leaves them to the host, the pending call completes, and the map is
    still the host-fed map -- as is an ordinary add after it"""
    host, dev = (new_map(ctx, fix, outlier_filter_min_points=min_points) for _ in range(2))
    store = CloudStore(ctx, capacity_points=1 << 14, max_clouds=16)
    key = 0
    for g in ("A", "B"):
        ping, special = pings[g], [np.zeros(2, np.float32)]
        for j, col in enumerate((0.5, 3.5, 40.5, 63.5, 100.5, len(ping.bearings) - 1.5)):
            p, dist = _near(ping, want_col=col, seed=j)
            assert dist < 1e-7, (g, col, dist)
            special.append(p)
        bearings = np.deg2rad(np.array(ping.bearings, np.float32) / 100)
        for j, end in enumerate((float(bearings[0]), float(bearings[-1]))):
            p, dist = _near(ping, want_angle=end, seed=10 + j)
            assert dist < float(np.spacing(np.float32(abs(end)))), (g, end, dist)
            special.append(p)
        for pts in (np.concatenate([np.array(special, np.float32), cloud(300, 77)[1:200]]), cloud(300, 78 + key)):
            h = store.put(pts)
            before = dev.feed_stats["undecided"]
            host.add_keyframe(key, Pose2(*POSES[key]), ping, store.read(h))
            dev.add_keyframe_store(key, Pose2(*POSES[key]), ping, store, h)
            same_stages(host, dev, (g, key))
            if len(pts) != 300:
                got = dev.feed_stats["undecided"] - before
                print("%s: undecided %d of %d points" % (g, got, len(pts)))
                assert got > 0
                if min_points == 1:                  # no filter: every boundary point got there (the origin is decided or
                    assert got >= 8                  # not by the table alone: its angle is 0)
            # nothing is left pending
            xy, pos = np.zeros((8, 2), np.float32), np.zeros(8, np.int32)
            assert dev._lib.sfe_map_measure_store_undecided(dev._h, _lib.ptr(xy, C.c_float), _lib.ptr(pos, C.c_int32), 8) \
                == _lib.SFE_ERR_ARG
            key += 1
    same_map(host, dev, "undecided points")
    for m in (host, dev):
        m.close()
    store.close()


@pytest.mark.parametrize("inflated", [False, True])
@pytest.mark.parametrize("feed", ["host", "store"])
def test_slots_on_demand_regrow_under_live_data(ctx, fix, pings, clouds, feed, inflated):
    """A Mapping keeps its slots on demand: the slot vector and the counts table of its one-map set grow when a slot past
    their end is asked for, while earlier slots hold cell lists.  Keys 0, 2 and 70, with key 70 in slot 70: the counts table
    starts with room for 66 slots, so it is reallocated (and every slot's counts pointer moved) while slots 0 and 1 are live;
    the third keyframe also grows the grid.  Then update_poses on the first and the last key in one call, and a frames=
    render of the two.  The grid, every keyframe's r / c / l, frames_grid() and the rendered occ equal, bit for bit, those of
    session 0 of a one-session MapBatch (whose slots lie in the arena) and of tests/mapping_ref.py given the same calls.

    The comparison with mapping_ref runs with inflation off (a 1 x 1 kernel): the polar image then holds only miss_prob, 0.5
    and hit_prob, the three values whose logit the device (double) and mapping_ref (scipy, float32) take to the same bits,
    so it can be bit for bit from points.  `inflated`: the fixture's inflation, many values per image; the device's log-odds
    are then within 2 ulp of mapping_ref's (test_gpu_mapping.py), so only the MapBatch is compared."""
    over = {} if inflated else dict(inflation_angle=0.0, inflation_range=0.0)
    m = new_map(ctx, fix, **over)
    b = MapBatch(ctx, 1, 8, max_pixels=8192, **dict(json.loads(str(fix["settings"])), **over))
    b.configure()
    others = [b.maps[0]] + ([] if inflated else [ref_map(fix, **over)])
    store = CloudStore(ctx, capacity_points=1 << 14, max_clouds=16)
    ping, keys = pings["A"], [0, 2, 70]

    def same_as(got, want, tag):
        want = np.asarray(want)
        cast = np.ascontiguousarray(want, got.dtype)
        assert np.array_equal(cast, want) and bits(got, cast), tag      # (the cast kept every value)

    def check(tag):
        for x in others:
            same_as(m.logodds_grid, x.logodds_grid, tag)
            for k in keys:
                for name in "rcl":
                    same_as(getattr(m.keyframes[k], name), getattr(x.keyframes[k], name), (tag, k, name))

    for key, p, pts in zip(keys, POSES, (clouds[0], clouds[1], clouds[4])):
        h = store.put(pts)
        if key == 70:
            # a keyframe's slot is len(keyframes) when it is added: with the missed keys filled in first, key 70 takes slot 70
            m.keyframes += [None] * (70 - len(m.keyframes))
        if feed == "store":
            m.add_keyframe_store(key, Pose2(*p), ping, store, h)
            b.add_keyframes_store([0], [key], [Pose2(*p)], ping, store, [h])
        else:
            m.add_keyframe(key, Pose2(*p), ping, store.read(h))
            b.add_keyframes([0], [key], [Pose2(*p)], ping, [store.read(h)])
        for ref in others[1:]:
            ref.add_keyframe(key, Pose2(*p), ping, store.read(h))
    assert [m.keyframes[k]._slot for k in keys] == [0, 1, 70] and len(m.keyframes) == 71
    assert m._grow[0] > 0 and m._grow[1] > 0                         # the third keyframe grew the grid
    if inflated:
        assert len(np.unique(m.keyframes[0].l)) > 3
    check("adds")
    new = [Pose2(POSES[i][0] + 0.7, POSES[i][1] - 1.1, POSES[i][2] + 0.2) for i in (0, 2)]
    m.update_poses([0, 70], new)
    b.update_poses([0, 0], [0, 70], new)
    for ref in others[1:]:
        for k, p in zip((0, 70), new):
            ref.update_pose(k, p)
    check("update_poses")
    got = m.get_occupancy_grid1(frames=[0, 70])
    frames = m.frames_grid()
    assert got.occ.size > 1000 and np.count_nonzero(frames) > 500
    for x in others:
        want = x.get_occupancy_grid1(frames=[0, 70])
        same_as(frames, x.frames_grid() if x is b.maps[0] else x.last_frames_grid, "frames grid")
        same_as(got.occ, want.occ, "occ")
    m.close()
    b.close()
    store.close()


def c_measure_store(m, store, slots, handles):
    """one sfe_map_measure_store call for the listed slots of map m (its current geometry), the whole protocol
    -> (points, undecided) per job"""
    n = len(slots)
    hr, hc = m._hit_halves()
    _, ktab, div = m._measure_args(np.zeros((0, 2), np.int32), hr, hc)
    i32 = lambda a: np.ascontiguousarray(np.array(a, np.int32))
    p32 = lambda a: _lib.ptr(a, C.c_int32)
    hit32, miss32 = np.float32(m.hit_prob), np.float32(m.miss_prob)
    n_pts, n_und = np.zeros(n, np.int32), np.zeros(n, np.int32)
    m._check(m._lib.sfe_map_measure_store(
        m._h, store.handle, n, p32(i32(slots)), p32(i32([m._geom] * n)), p32(i32(handles)), p32(i32([m._hit_table()] * n)),
        float(m.outlier_filter_radius), int(m.outlier_filter_min_points), p32(i32([(hr, hc)] * n)), p32(i32([0] * n)),
        _lib.ptr(ktab, C.c_float), len(ktab), _lib.ptr(np.full(n, div, np.float64), C.c_double), float(miss32),
        float(logit(miss32)), float(hit32), float(logit(hit32)), p32(n_pts), p32(n_und)))
    total = int(n_und.sum())
    if total:
        xy, pos = np.zeros((total, 2), np.float32), np.zeros(total, np.int32)
        m._check(m._lib.sfe_map_measure_store_undecided(m._h, _lib.ptr(xy, C.c_float), p32(pos), total))
        assert np.all(np.diff(pos) > 0)
        cells = np.ascontiguousarray(m._hit_indices(xy)[0], np.int32)
        m._check(m._lib.sfe_map_measure_store_finish(m._h, total, p32(pos), p32(cells)))
    return list(n_pts), list(n_und)


@pytest.mark.parametrize("special", [False, True])
def test_several_keyframes_in_one_c_call(ctx, fix, pings, clouds, special):
    """sfe_map_measure_store with n = 3 (slots of one map, one of the clouds empty) == three calls with n = 1: the images of
    the three slots and the stages of every job; `special`: with undecided points in one of the clouds"""
    ping = pings["B"]
    store = CloudStore(ctx, capacity_points=1 << 14, max_clouds=16)
    first = store.put(clouds[1])
    pts = [clouds[0], clouds[2], clouds[4]]
    if special:
        pts[2] = np.concatenate([clouds[4][:700], np.array([_near(ping, want_col=40.5, seed=2)[0]], np.float32)])
    handles = [store.put(p) for p in pts]
    assert [len(p) for p in pts][1] == 0
    one, three = new_map(ctx, fix), new_map(ctx, fix)
    for m in (one, three):
        m.add_keyframe_store(0, Pose2(0.0, 0.0, 0.0), ping, store, first)      # the geometry and the hit table
    n_px = int(np.prod(one.oculus_image_size))
    got = c_measure_store(three, store, [1, 2, 3], handles)
    stages = []
    for b in range(3):
        hits, prob = np.zeros(one.oculus_image_size, np.uint8), np.zeros(one.oculus_image_size, np.float32)
        fh = np.zeros(one.oculus_image_size[1], np.int32)
        three._check(three._lib.sfe_map_measure_stages(three._h, b, _lib.ptr(hits, C.c_uint8), _lib.ptr(prob, C.c_float),
                                                       _lib.ptr(fh, C.c_int32)))
        stages.append((hits, prob, fh))
    want = [[], []]
    for b in range(3):
        p, u = c_measure_store(one, store, [1 + b], [handles[b]])
        want[0] += p
        want[1] += u
        for x, y in zip(stages[b], one.measure_stages()):
            assert bits(x, y), b
        assert bits(three._read_logodds(1 + b, n_px), one._read_logodds(1 + b, n_px)), b
    assert got == (want[0], want[1]) and got[0] == [len(p) for p in pts]
    assert (sum(got[1]) > 0) or not special
    assert np.count_nonzero(stages[0][0]) > 100 and np.count_nonzero(stages[1][0]) == 0
    # a slot twice in one call is refused
    i32 = lambda *a: _lib.ptr(np.array(a, np.int32), C.c_int32)
    out = np.zeros(4, np.int32)
    hr, hc = one._hit_halves()
    _, ktab, div = one._measure_args(np.zeros((0, 2), np.int32), hr, hc)
    rc = one._lib.sfe_map_measure_store(
        one._h, store.handle, 2, i32(4, 4), i32(one._geom, one._geom), i32(handles[0], handles[2]), i32(0, 0), 2.0, 8,
        i32(hr, hc, hr, hc), i32(0, 0), _lib.ptr(ktab, C.c_float), len(ktab), _lib.ptr(np.full(2, div), C.c_double), 0.3,
        -0.8, 0.8, 1.4, _lib.ptr(out[:2], C.c_int32), _lib.ptr(out[2:], C.c_int32))
    assert rc == _lib.SFE_ERR_ARG
    for m in (one, three):
        m.close()
    store.close()


def test_refusals_change_nothing(ctx, fix, pings, clouds, monkeypatch):
    """a dead handle, a store of another context, an image the device cannot hold and a slot that holds another image each
    raise, and the map is as it was -- the sonar settings, the skips, the geometry id and the counters included"""
    store = CloudStore(ctx, capacity_points=1 << 14, max_clouds=16)
    handles = [store.put(clouds[i]) for i in (0, 1, 4)]
    m, host = new_map(ctx, fix, pub_occupancy2=True), new_map(ctx, fix, pub_occupancy2=True)
    # ... at the first keyframe of all
    before = snapshot(m)
    for bad in (len(store), -1):
        with pytest.raises(_lib.SonarFEError, match="cloud %d named" % bad):
            m.add_keyframe_store(0, Pose2(*POSES[0]), pings["A"], store, bad)
        assert snapshot(m) == before and m._geom == -1 and m.oculus.num_ranges is None
    m.add_keyframe_store(0, Pose2(*POSES[0]), pings["A"], store, handles[0])
    before = snapshot(m)
    # a handle that store.truncate dropped, with a ping that brings another geometry
    dead = store.put(clouds[3])
    store.truncate(dead)
    with pytest.raises(_lib.SonarFEError, match="cloud %d named" % dead):
        m.add_keyframe_store(1, Pose2(*POSES[1]), pings["B"], store, dead)
    assert snapshot(m) == before
    # a store of another context: refused here, and by the device on its own
    other_ctx = _lib.Context(ctx.device)
    other = CloudStore(other_ctx, capacity_points=1 << 12, max_clouds=4)
    h_other = other.put(clouds[1])
    with pytest.raises(ValueError, match="another context"):
        m.add_keyframe_store(1, Pose2(*POSES[1]), pings["B"], other, h_other)
    assert snapshot(m) == before
    i32 = lambda *a: _lib.ptr(np.array(a, np.int32), C.c_int32)
    hr, hc = m._hit_halves()
    _, ktab, div = m._measure_args(np.zeros((0, 2), np.int32), hr, hc)
    out = np.zeros(2, np.int32)
    call = lambda st, slot, geom, handle, tab: m._lib.sfe_map_measure_store(
        m._h, st.handle, 1, i32(slot), i32(geom), i32(handle), i32(tab), 2.0, 8, i32(hr, hc), i32(0),
        _lib.ptr(ktab, C.c_float), len(ktab), _lib.ptr(np.full(1, div), C.c_double), 0.3, -0.8, 0.8, 1.4,
        _lib.ptr(out[:1], C.c_int32), _lib.ptr(out[1:], C.c_int32))
    assert call(other, 1, m._geom, h_other, 0) == _lib.SFE_ERR_ARG
    assert call(store, 1, m._geom, handles[1], 5) == _lib.SFE_ERR_ARG          # an unknown table
    assert call(store, 1, 99, handles[1], 0) == _lib.SFE_ERR_ARG               # an unknown geometry
    assert call(store, -1, m._geom, handles[1], 0) == _lib.SFE_ERR_ARG
    assert snapshot(m) == before
    other.close()
    # An image the map cannot hold.  An sfe_map has no arena: the one image it refuses is one of 2^30 pixels or more, which
    # no test can build; so the geometry is offered to the device with that size (the table is not read before the refusal).
    # What is under test is that the refusal, raised inside _new_keyframe after the ping's geometry was taken, leaves
    # the sonar settings and the skips as they were.
    real = m._register_geometry
    with monkeypatch.context() as mp:
        mp.setattr(m, "_register_geometry", lambda xy, shape: real(xy, (1 << 15, 1 << 15)))
        with pytest.raises(_lib.SonarFEError):
            m.add_keyframe_store(1, Pose2(*POSES[1]), pings["B"], store, handles[1])
    assert snapshot(m) == before
    # ... and a slot that holds the 6656 pixels of geometry A cannot take the 8192 of geometry B: sfe_map_measure's refusal
    m.add_keyframe_store(1, Pose2(*POSES[1]), pings["B"], store, handles[1])
    before = snapshot(m)
    assert sorted(m._geom_shape.values()) == [(52, 128), (64, 128)]
    assert call(store, 0, m._geom, handles[1], 1) == _lib.SFE_ERR_ARG
    assert snapshot(m) == before
    # the next valid add, and the map of the valid adds alone
    m.add_keyframe_store(2, Pose2(*POSES[2]), pings["A"], store, handles[2])
    for k, (g, h) in enumerate(zip("ABA", handles)):
        host.add_keyframe(k, Pose2(*POSES[k]), pings[g], store.read(h))
    same_map(host, m, "after the refusals")
    assert m.feed_stats["calls"] == 3
    for x in (m, host):
        x.close()
    store.close()


def test_point_cloud_is_read_from_the_store_on_access(ctx, fix, pings, clouds, monkeypatch):
    store = CloudStore(ctx, capacity_points=1 << 14, max_clouds=16)
    handles = [store.put(clouds[i]) for i in (1, 3)]
    reads = []
    real = store.read
    monkeypatch.setattr(store, "read", lambda h: (reads.append(h), real(h))[1])
    m = new_map(ctx, fix, pub_occupancy2=True)
    assert m.point_cloud is None
    m.add_keyframe_store(0, Pose2(*POSES[0]), pings["A"], store, handles[0])
    assert reads == [] and m._point_cloud is None and m._cloud_ref == (store, handles[0])       # no eager copy
    got = m.point_cloud
    assert reads == [handles[0]] and got.dtype == np.float32 and np.array_equal(got, clouds[1])
    m.add_keyframe(1, Pose2(*POSES[1]), pings["A"], clouds[3])          # the host route keeps what it was handed
    assert m.point_cloud is clouds[3]
    m.add_keyframe_store(2, Pose2(*POSES[2]), pings["A"], store, handles[1])
    assert np.array_equal(m.point_cloud, clouds[3]) and m.point_cloud is not clouds[3]
    m.point_cloud = None                                                 # assigning keeps working
    assert m.point_cloud is None and m._cloud_ref is None
    off = new_map(ctx, fix, pub_occupancy2=False)
    reads.clear()
    off.add_keyframe_store(0, Pose2(*POSES[0]), pings["A"], store, handles[0])
    assert off.point_cloud is None and off._cloud_ref is None and reads == []
    for x in (m, off):
        x.close()
    store.close()


def test_front_end_feeds_its_map(ctx, shipped_cfar):
    """replay.FrontEnd(mapping=...): the records of mapping=None whatever the feed; the two maps equal each other and the map
    of a one-session SessionBatch on the same pings"""
    from test_global_init import _product_fe, _replay_session, _session
    from sonar_slam_amd import chained, icp_config
    from sonar_slam_amd.feature_extraction import SonarPing, oculus_bearings
    K, ROWS = 4, 256
    frames, _, dr, _, bearings, _ = _session(K, rows=ROWS, step=1.7, turn=0.3, seed=21, n_world=9000, start=(20.0, 0.0, 0.0))
    ping = SonarPing(frames[0], oculus_bearings(frames.shape[-1]), 30.0 / ROWS)
    settings = dict(x0=0.0, y0=-20.0, width=40.0, height=40.0, inc=25.0)

    def run(mapping):
        store = CloudStore(ctx, capacity_points=1 << 18, max_clouds=64)
        front, log = _replay_session(ctx, frames, bearings, dr, ROWS, store, ssm_min_points=20, ssm_initialization=False,
                                     mapping=mapping)
        assert len(log) == K and len(store) == K
        return front, copy.deepcopy(log), store

    plain, plain_log, s0 = run(None)
    host, host_log, s1 = run(dict(ping=ping, feed="host", **settings))
    dev, dev_log, s2 = run(dict(ping=ping, feed="store", **settings))
    assert plain.map is None and isinstance(host.map, Mapping) and host.map.ctx is ctx
    _same_records(host_log, plain_log)
    _same_records(dev_log, plain_log)
    same_map(host.map, dev.map, "front end")
    assert len(dev.map.keyframes) == K and np.count_nonzero(dev.map.logodds_grid) > 1000
    stats = dev.map.feed_stats
    print("undecided %d of %d points" % (stats["undecided"], stats["points"]))
    assert stats["calls"] == K and stats["points"] > 1000 and stats["undecided"] <= 0.01 * stats["points"]
    assert host.map.feed_stats["calls"] == 0
    # the one-session batch on the same pings
    fe = _product_fe(ctx)
    fe.generate_map_xy(ping)
    sb = chained.SessionBatch(ctx, fe.geometry, shipped_cfar.params["SOCA"], "SOCA", 65, icp_config.shipped_params(), 1, K,
                              dr[None], ssm_min_points=20, mapping=dict(ping=ping, max_pixels=1 << 16, feed="store", **settings))
    for k in range(K):
        sb.upload_frames(k, frames[None, k])
    recs = sb.run()
    for k in range(K):
        assert tuple(recs[k]["pose"][0]) == dev_log[k]["pose"], k
    same(sb.maps.maps[0], dev.map, "one-session batch")
    assert sb.maps.feed_stats == dev.map.feed_stats
    sb.free()
    for front, store in ((plain, s0), (host, s1), (dev, s2)):
        if front.map is not None:
            front.map.close()
        store.close()
