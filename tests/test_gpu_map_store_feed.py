"""MapBatch.add_keyframes_store: the occupancy maps fed from a CloudStore on the device are, bit for bit, the maps
add_keyframes builds from store.read_many(handles) -- hit masks, polar images, cell lists, grids, boxes and origins."""
import copy
import json
import os
import sys

import ctypes as C
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]
import mapping_ref  # noqa: E402
from test_gpu_map_batch import _same_records, digest  # noqa: E402
from sonar_slam_amd import _lib  # noqa: E402
from sonar_slam_amd import mapping  # noqa: E402
from sonar_slam_amd.mapping import MapBatch  # noqa: E402
from sonar_slam_amd.pose2 import Pose2  # noqa: E402
from sonar_slam_amd.store import CloudStore  # noqa: E402

pytestmark = pytest.mark.gpu

FIX = os.path.join(HERE, "golden", "mapping_session.npz")
S, STEPS = 3, 5
# around outlier_filter_min_points = 20 (a cluster of 19 or 20 is emptied by the filter, one of 21 stays); 1500 crosses a
# 256-thread block of the per-point kernels and a 1024-point chunk
COUNTS = [0, 1, 19, 20, 21, 300, 1500]


@pytest.fixture(scope="module")
def fix():
    return np.load(FIX)


@pytest.fixture(scope="module")
def pings(fix):
    geoms = json.loads(str(fix["geoms"]))       # A: 128 beams x 256 ranges (r_skip 5), B: 256 x 128 (r_skip 2, c_skip 2)
    return {g: mapping_ref.SessionPing(*geoms[g]) for g in ("A", "B")}


def cloud(n, seed):
    """n float32 points: small ones a tight cluster; large ones all over and beyond the 10.24 m, +-65 degree fan, with a
    point at the origin"""
    rng = np.random.default_rng(seed)
    if n <= 21:
        return (np.array([6.0, 1.0]) + rng.uniform(-0.4, 0.4, (n, 2))).astype(np.float32)
    rho, b = rng.uniform(0.05, 12.0, n), rng.uniform(-1.3, 1.3, n)
    pts = np.c_[rho * np.cos(b), rho * np.sin(b)].astype(np.float32)
    pts[0] = 0.0
    assert (np.abs(b) > np.deg2rad(65)).any() and (rho > 10.24).any()
    return pts


@pytest.fixture(scope="module")
def clouds():
    """[step][session]: every size of COUNTS, and a cloud of 21 scattered points, which the filter empties"""
    out = [[cloud(COUNTS[(S * k + s) % len(COUNTS)], 10 * k + s) for s in range(S)] for k in range(STEPS)]
    rng = np.random.default_rng(3)
    out[STEPS - 1][S - 1] = (np.c_[np.arange(21) * 0.45 - 4.0, 3.0 + 3.0 * (np.arange(21) % 2)]
                             + rng.uniform(0, 0.01, (21, 2))).astype(np.float32)
    assert sorted({len(c) for row in out for c in row}) == COUNTS
    return out


def batch(ctx, fix, n=S, max_keyframes=6, max_pixels=8192, **over):
    b = MapBatch(ctx, n, max_keyframes, max_pixels=max_pixels, **dict(json.loads(str(fix["settings"])), **over))
    b.configure()
    return b


def pose(s, k):
    return Pose2(2.5 * k + s, -2.0 * k + 0.5 * s, 0.3 * k - 0.2 * s)


def same_step(a, b, tag):
    """the measurement of every job of the last add call"""
    for s, (va, vb) in enumerate(zip(a.maps, b.maps)):
        assert va._meas_job == vb._meas_job, tag
        if va._meas_job < 0:
            continue
        for x, y in zip(va.measure_stages(), vb.measure_stages()):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (tag, s)


def same_maps(a, b, tag):
    for s, (va, vb) in enumerate(zip(a.maps, b.maps)):
        assert np.array_equal(va.logodds_grid.view(np.int32), vb.logodds_grid.view(np.int32)), (tag, s)
        assert (va.rmin, va.rmax, va.cmin, va.cmax) == (vb.rmin, vb.rmax, vb.cmin, vb.cmax), (tag, s)
        assert (va.x0, va.y0, va.rows, va.cols, va._grow) == (vb.x0, vb.y0, vb.rows, vb.cols, vb._grow), (tag, s)
        assert va.device_shape() == vb.device_shape() and len(va.keyframes) == len(vb.keyframes), (tag, s)
        for k, (ka, kb) in enumerate(zip(va.keyframes, vb.keyframes)):
            assert (ka is None) == (kb is None)
            if ka is None:
                continue
            assert (ka.box, ka.base, ka.geom) == (kb.box, kb.base, kb.geom), (tag, s, k)
            for name in ("r", "c", "l", "logodds"):
                x, y = getattr(ka, name), getattr(kb, name)
                assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (tag, s, k, name)
    assert digest(a) == digest(b), tag


def feed_both(ctx, fix, steps, **over):
    """`steps`: [(ping, [cloud per session])] -> (host-fed batch, store-fed batch), compared after every step"""
    host, dev = batch(ctx, fix, **over), batch(ctx, fix, **over)
    store = CloudStore(ctx, capacity_points=1 << 16, max_clouds=64)
    for k, (ping, row) in enumerate(steps):
        handles = [store.put(c) for c in row]
        args = (list(range(S)), [k] * S, [pose(s, k) for s in range(S)], ping)
        host.add_keyframes(*args, store.read_many(handles))
        dev.add_keyframes_store(*args, store, handles)
        same_step(host, dev, "step %d" % k)
    return host, dev, store


@pytest.mark.parametrize("min_points", [20, 1])
@pytest.mark.parametrize("geoms", ["A", "B", "AB"])
def test_store_fed_maps_are_the_host_fed_maps(ctx, fix, pings, clouds, min_points, geoms):
    steps = [(pings[geoms[k % len(geoms)]], clouds[k]) for k in range(STEPS)]
    host, dev, store = feed_both(ctx, fix, steps, outlier_filter_min_points=min_points)
    same_maps(host, dev, "%s, min_points %d" % (geoms, min_points))
    # an empty cloud is a keyframe without a measurement; a cloud the filter empties keeps its kernel: all of its pixels
    # are 0.5 before the columns, and the first "hit" of every column is the image's height either way
    stats = dev.feed_stats
    assert stats["calls"] == STEPS and stats["points"] == sum(len(c) for row in clouds for c in row)
    print("undecided %d of %d points" % (stats["undecided"], stats["points"]))
    assert stats["undecided"] <= 0.01 * stats["points"]
    assert host.feed_stats == {"points": 0, "undecided": 0, "calls": 0}
    assert np.count_nonzero(dev.maps[0].logodds_grid) > 500
    for b in (host, dev):
        b.close()
    store.close()


def _near(ping, want_angle=None, want_col=None, tries=4000, seed=0):
    """a float32 point of the fan whose angle (double atan2) is as close as float32 coordinates allow to `want_angle`, or
    whose column value (the table, in double) to `want_col` -> (point, distance)"""
    o = mapping._Oculus()
    o.configure(ping)
    breaks, coef = mapping.spline_table(o)
    if want_angle is None:
        lo, hi = float(o.bearings[0]), float(o.bearings[-1])
        for _ in range(80):                      # the table is increasing
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if float(o.b2c(mid)) < want_col else (lo, mid)
        want_angle = lo
    rho = np.random.default_rng(seed).uniform(2.0, 9.0, tries)
    pts = np.c_[rho * np.cos(want_angle), rho * np.sin(want_angle)].astype(np.float32)
    a = np.arctan2(pts[:, 1].astype(np.float64), pts[:, 0].astype(np.float64))
    if want_col is None:
        dist = np.abs(a - want_angle)
    else:
        k = np.clip(np.searchsorted(breaks, a, side="right") - 1, 0, len(coef) - 1)
        d = a - breaks[k]
        dist = np.abs(((coef[k, 0] * d + coef[k, 1]) * d + coef[k, 2]) * d + coef[k, 3] - want_col)
    i = int(np.argmin(dist))
    return pts[i], float(dist[i])


@pytest.mark.parametrize("min_points", [8, 1])
def test_undecided_points_take_the_host_route(ctx, fix, pings, min_points):
    """points on a rounding boundary of the bearing column (within 1e-7 columns of x.5) and on both ends of the bearing table
    (within a float32 ulp): the device leaves them to the host, and the maps are still the host-fed maps"""
    rows = []
    for g in ("A", "B"):
        ping, special = pings[g], []
        for j, col in enumerate((0.5, 3.5, 40.5, 63.5, 100.5, len(ping.bearings) - 1.5)):
            p, dist = _near(ping, want_col=col, seed=j)
            assert dist < 1e-7, (g, col, dist)
            special.append(p)
        bearings = np.deg2rad(np.array(ping.bearings, np.float32) / 100)
        for j, end in enumerate((float(bearings[0]), float(bearings[-1]))):
            p, dist = _near(ping, want_angle=end, seed=10 + j)
            assert dist < float(np.spacing(np.float32(abs(end)))), (g, end, dist)
            special.append(p)
        base = cloud(300, 77)
        rows.append((ping, [np.concatenate([np.array(special, np.float32), base[: 100 * (s + 1)]]) for s in range(S)]))
    host, dev, store = feed_both(ctx, fix, rows, outlier_filter_min_points=min_points)
    same_maps(host, dev, "undecided points")
    stats = dev.feed_stats
    print("undecided %d of %d points" % (stats["undecided"], stats["points"]))
    assert stats["undecided"] > 0
    if min_points == 1:                          # no filter: every special point of every session and step got there
        assert stats["undecided"] >= 2 * S * 8
    for b in (host, dev):
        b.close()
    store.close()


def test_refusals_change_nothing(ctx, fix, pings, clouds):
    """a handle the store does not hold, a slot beyond max_keyframes and an image above max_pixels each raise, and the
    batch is as it was"""
    store = CloudStore(ctx, capacity_points=1 << 14, max_clouds=16)
    handles = [store.put(clouds[1][s]) for s in range(S)]
    b = batch(ctx, fix, max_keyframes=2)
    args = lambda k, ping=pings["A"]: (list(range(S)), [k] * S, [pose(s, k) for s in range(S)], ping, store)
    # ... at the first keyframe of all
    before = digest(b)
    for bad in (len(store), len(store) + 7, -1):
        with pytest.raises(_lib.SonarFEError, match="cloud %d named" % bad):
            b.add_keyframes_store(*args(0), [handles[0], bad, handles[2]])
        assert digest(b) == before and b.maps[0]._geom == -1
    b.add_keyframes_store(*args(0), handles)
    before = digest(b)
    with pytest.raises(_lib.SonarFEError, match="cloud %d named" % len(store)):
        b.add_keyframes_store(*args(1, pings["B"]), [handles[0], handles[1], len(store)])
    assert digest(b) == before
    b.add_keyframes_store(*args(1), handles)
    before = digest(b)
    with pytest.raises(_lib.SonarFEError, match="max_keyframes = 2"):
        b.add_keyframes_store(*args(2), handles)
    assert digest(b) == before
    # the device refuses a slot beyond the arena on its own
    i32 = lambda *a: _lib.ptr(np.array(a, np.int32), C.c_int32)
    out = np.zeros(2, np.int32)
    rc = b._lib.sfe_mapset_measure_store(
        b._h, store.handle, 1, i32(0), i32(2), i32(0), i32(handles[0]), i32(0), 2.0, 8, i32(1, 1), i32(0),
        _lib.ptr(np.ones(9, np.float32), C.c_float), 9, _lib.ptr(np.ones(1), C.c_double), 0.3, -0.8, 0.8, 1.4,
        _lib.ptr(out[:1], C.c_int32), _lib.ptr(out[1:], C.c_int32))
    assert rc == _lib.SFE_ERR_CAP and digest(b) == before
    small = batch(ctx, fix, max_keyframes=2, max_pixels=7000)
    small.add_keyframes_store(*args(0), handles)                       # geometry A: 6656 pixels
    before = digest(small)
    with pytest.raises(_lib.SonarFEError, match="room for 7000 pixels"):
        small.add_keyframes_store(*args(1, pings["B"]), handles)       # geometry B: 8192 pixels
    assert digest(small) == before
    small.add_keyframes_store(*args(1), handles)
    other = batch(ctx, fix, max_keyframes=2)
    for k in range(2):
        other.add_keyframes(list(range(S)), [k] * S, [pose(s, k) for s in range(S)], pings["A"], store.read_many(handles))
    same_maps(other, small, "after the refusals")
    same_maps(other, b, "after the refusals")
    for x in (b, small, other):
        x.close()
    store.close()


def test_point_cloud_is_read_from_the_store_on_access(ctx, fix, pings, clouds):
    store = CloudStore(ctx, capacity_points=1 << 14, max_clouds=16)
    handles = [store.put(clouds[1][s]) for s in range(S)]
    b = batch(ctx, fix, pub_occupancy2=True)
    assert all(v.point_cloud is None for v in b.maps)
    b.add_keyframes_store([2, 0], [0, 0], [pose(2, 0), pose(0, 0)], pings["A"], store, [handles[2], handles[0]])
    for s in (0, 2):
        v = b.maps[s]
        assert v._point_cloud is None and v._cloud_ref == (store, handles[s])         # no eager copy
        got = v.point_cloud
        assert got.dtype == np.float32 and np.array_equal(got, store.read(handles[s])) and np.array_equal(got, clouds[1][s])
    assert b.maps[1].point_cloud is None
    pts = clouds[2][0]
    b.add_keyframes([0], [1], [pose(0, 1)], pings["A"], [pts])        # the host route keeps what it was handed
    assert b.maps[0].point_cloud is pts
    off = batch(ctx, fix, pub_occupancy2=False)
    off.add_keyframes_store([0], [0], [pose(0, 0)], pings["A"], store, [handles[0]])
    assert off.maps[0].point_cloud is None
    for x in (b, off):
        x.close()
    store.close()


def test_session_batch_feeds_its_maps_from_the_store(ctx, shipped_cfar):
    """SessionBatch(mapping=dict(feed="store")): the records and every session's map of feed="host"; one feed call per step"""
    from test_global_init import _product_fe, _session
    from sonar_slam_amd import chained, icp_config
    from sonar_slam_amd.feature_extraction import SonarPing, oculus_bearings
    K, ROWS, n = 5, 256, 3
    sess = [_session(K, rows=ROWS, step=1.7, turn=0.3, seed=21 + 4 * s, n_world=9000, start=(20.0 - 1.5 * s, 0.8 * s, 0.1 * s))
            for s in range(n)]
    frames, dr = np.stack([x[0] for x in sess]), np.stack([x[2] for x in sess])
    ping = SonarPing(frames[0][0], oculus_bearings(frames.shape[-1]), 30.0 / ROWS)
    settings = dict(x0=0.0, y0=-20.0, width=40.0, height=40.0, inc=25.0)

    def run(feed):
        fe = _product_fe(ctx)
        fe.generate_map_xy(ping)
        sb = chained.SessionBatch(ctx, fe.geometry, shipped_cfar.params["SOCA"], "SOCA", 65, icp_config.shipped_params(), n, K, dr,
                                  ssm_min_points=20, mapping=dict(ping=ping, max_pixels=1 << 16, feed=feed, **settings))
        for k in range(K):
            sb.upload_frames(k, frames[:, k])
        return sb, copy.deepcopy(sb.run()), copy.deepcopy(sb.loops)

    host, host_recs, host_loops = run("host")
    dev, dev_recs, dev_loops = run("store")
    _same_records(dev_recs, host_recs)
    assert dev_loops == host_loops
    same_maps(host.maps, dev.maps, "whole session")
    stats = dev.maps.feed_stats
    print("undecided %d of %d points" % (stats["undecided"], stats["points"]))
    assert stats["calls"] == K and stats["points"] > 1000 and stats["undecided"] <= 0.01 * stats["points"]
    assert host.maps.feed_stats["calls"] == 0
    assert np.count_nonzero(dev.maps.maps[0].logodds_grid) > 1000
    dev.reset()
    assert dev.maps.feed_stats == {"points": 0, "undecided": 0, "calls": 0}
    host.free()
    dev.free()
