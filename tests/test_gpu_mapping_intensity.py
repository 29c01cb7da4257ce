"""The intensity mosaic on the device (sonar_slam_amd.mapping with pub_intensity and intensity_skips="oculus";
csrc/sfe_map.hip) against the reference's recorded session (tests/golden/intensity_session.npz, written by the reference's
own mapping.py) and against tests/intensity_ref.py where the reference cannot run (column growth)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import intensity_ref  # noqa: E402
import mapping_ref  # noqa: E402
import oracle  # noqa: E402
from intensity_ref import sha  # noqa: E402
from sonar_slam_amd import _lib  # noqa: E402
from sonar_slam_amd.mapping import DeviceImage, MapBatch, Mapping  # noqa: E402
from sonar_slam_amd.pose2 import Pose2  # noqa: E402

pytestmark = pytest.mark.gpu

ON = dict(pub_intensity=True, intensity_skips="oculus")


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(HERE, "golden", "intensity_session.npz"))


@pytest.fixture(scope="module")
def map_fix():
    return np.load(os.path.join(HERE, "golden", "mapping_session.npz"))


def configured(m, settings, **over):
    for k, v in dict(settings, **over).items():
        setattr(m, k, v)
    m.configure()
    return m


def ref_map(settings, **over):
    m = intensity_ref.Mapping()
    m.remove_outlier = oracle.remove_outlier
    return configured(m, {k: v for k, v in settings.items() if k != "pub_intensity"}, **over)


def live(m):
    return [kf for kf in m.keyframes if kf is not None]


def sums_hold(m):
    """counter_grid.sum() == sum of len(kf.r), intensity_grid.sum() == sum of kf.i.sum()"""
    inten, count = m.intensity_grid, m.counter_grid
    assert inten.dtype == np.uint32 and count.dtype == np.uint16 and inten.shape == count.shape == (m.rows, m.cols)
    assert int(count.sum(dtype=np.int64)) == sum(len(kf.r) for kf in live(m))
    assert int(inten.sum(dtype=np.int64)) == sum(int(kf.i.sum(dtype=np.int64)) for kf in live(m))
    return inten, count


def same_map(m, ref, tag=None):
    """a product map against a restatement (or another product map): box, origin, size, both grids, every keyframe's i"""
    assert [int(m.rmin), int(m.rmax), int(m.cmin), int(m.cmax), m.rows, m.cols, m.x0, m.y0] == \
        [int(ref.rmin), int(ref.rmax), int(ref.cmin), int(ref.cmax), ref.rows, ref.cols, ref.x0, ref.y0], tag
    assert np.array_equal(m.intensity_grid, ref.intensity_grid), tag
    assert np.array_equal(m.counter_grid, ref.counter_grid), tag
    assert len(m.keyframes) == len(ref.keyframes), tag
    for kf, rk in zip(m.keyframes, ref.keyframes):
        assert (kf is None) == (rk is None), tag
        if kf is not None:
            i = kf.i
            assert i.dtype == np.uint8 and np.array_equal(i, rk.i), tag
            assert np.array_equal(kf.r, rk.r) and np.array_equal(kf.c, rk.c), tag


def same_pub(got, want):
    assert intensity_ref.info_of(got) == intensity_ref.info_of(want)
    assert np.array_equal(np.array(got.data, np.int8), np.array(want.data, np.int8))
    assert got.occ.dtype == np.int8 and got.occ.shape == (got.info.height, got.info.width)
    assert got.header.frame_id == "map" and got.info.origin.orientation.w == 1


def digest(m):
    """what a refused call must leave as it was"""
    return (sha(m.intensity_grid), sha(m.counter_grid), sha(m.logodds_grid), len(m.keyframes), m.rmin, m.rmax, m.cmin, m.cmax,
            m.rows, m.cols, m._geom, m.oculus_image_size, m.oculus_r_skip, m.oculus_c_skip)


@pytest.fixture(scope="module")
def reference_run(ctx, fix, map_fix):
    """the recorded session through Mapping, from points, checked against the reference after every step (once for the
    module; the tests that need its end state leave it unchanged)"""
    settings, geoms, steps, points, _ = intensity_ref.fixture_session(fix, map_fix)
    m = configured(Mapping(ctx), settings, intensity_skips="oculus")
    seen = []

    def check(i, st):
        inten, count = sums_hold(m)
        got = dict(box=[int(m.rmin), int(m.rmax), int(m.cmin), int(m.cmax)], x0=float(m.x0), y0=float(m.y0), rows=int(m.rows),
                   cols=int(m.cols), intensity=sha(inten), counter=sha(count), i=intensity_ref.kf_i_digest(m))
        for k, v in got.items():
            assert v == st[k], (i, st["op"], st.get("key"), k)
        if st["op"] == "add":
            kf = m.keyframes[st["key"]]
            nb, nr, _ = geoms[st["geom"]]
            image = intensity_ref.pattern_ping(st["key"], nr, nb)
            assert np.array_equal(kf.intensity, image[::st["skips"][0], ::st["skips"][1]].ravel())
        last = i + 1 == len(steps) or steps[i + 1].get("pass_") != st.get("pass_")
        tag = {"add": "adds"}.get(st["op"], st.get("pass_"))
        if last and "intensity_%s" % tag in fix:
            box = (slice(m.rmin, m.rmax + 1), slice(m.cmin, m.cmax + 1))
            assert np.array_equal(inten[box], fix["intensity_%s" % tag]) and np.array_equal(count[box], fix["counter_%s" % tag])
            for k in (0, 7, 19):
                assert np.array_equal(m.keyframes[k].i, fix["i_%s_%d" % (tag, k)])
        seen.append(i)

    intensity_ref.replay(m, steps, geoms, points, Pose2, check=check)
    assert seen == list(range(len(steps)))
    return m


def test_reference_session_from_points(ctx, fix, map_fix, reference_run):
    """after every step both grids' digests and every keyframe's i (the fixture above), then the published image and its
    info, are bit for bit the reference's; the log-odds grid is the one the same map builds without the mosaic"""
    m = reference_run
    msg = m.get_intensity_grid()
    assert np.array_equal(np.array(msg.data, np.int8), fix["pub_data"])
    assert intensity_ref.info_of(msg) == list(fix["pub_info"])
    assert msg.occ.shape == (msg.info.height, msg.info.width) and msg.header.frame_id == "map"
    settings, geoms, steps, points, _ = intensity_ref.fixture_session(fix, map_fix)
    plain = configured(Mapping(ctx), settings, pub_intensity=False)
    assert plain.intensity_grid is None and plain.counter_grid is None
    for st in steps:
        if st["op"] == "add":
            plain.add_keyframe(st["key"], Pose2(*st["pose"]), mapping_ref.SessionPing(*geoms[st["geom"]]),
                               np.asarray(points[st["key"]], np.float64))
        else:
            plain.update_pose(st["key"], Pose2(*st["pose"]))
    assert np.array_equal(plain.logodds_grid.view(np.int32), m.logodds_grid.view(np.int32))
    assert plain.keyframes[0].i is None and plain.keyframes[0].intensity is None
    with pytest.raises(NotImplementedError, match="get_intensity_grid"):
        plain.get_intensity_grid()


def test_reference_session_batched_from_logodds(ctx, fix, map_fix):
    """the same session with ping.ping instead of image=, the reference's log-odds images and each pose pass as one
    update_poses call (the growth then falls in the middle of a batch): the digests at the end of every pass, and the
    log-odds grid of the restatement's run of these settings, bit for bit"""
    settings, geoms, steps, points, logodds = intensity_ref.fixture_session(fix, map_fix)
    m = configured(Mapping(ctx), settings, intensity_skips="oculus")
    with pytest.raises(RuntimeError, match="no keyframe"):
        m.get_intensity_grid()

    def check(i, st):
        inten, count = sums_hold(m)
        assert (sha(inten), sha(count), intensity_ref.kf_i_digest(m)) == (st["intensity"], st["counter"], st["i"]), i
        assert [int(m.rmin), int(m.rmax), int(m.cmin), int(m.cmax), m.rows, m.cols] == st["box"] + [st["rows"], st["cols"]]

    intensity_ref.replay(m, steps, geoms, points, Pose2, check=check, batched=True, image_kw=False, logodds=logodds)
    ref = ref_map(settings)
    intensity_ref.replay(ref, steps, geoms, points, Pose2, logodds=logodds)
    same_map(m, ref)
    assert np.array_equal(m.logodds_grid.view(np.int32), ref.logodds_grid.view(np.int32))
    same_pub(m.get_intensity_grid(), ref.get_intensity_grid())
    assert np.array_equal(np.array(m.get_intensity_grid().data, np.int8), fix["pub_data"])


@pytest.mark.parametrize("width", [20.0, 20.2])
def test_growth_on_all_four_sides(ctx, map_fix, width):
    """the 20 m map of mapping_session.npz grows by 6 m steps on all four sides, in the middle of a pose pass too: on the
    left and right the reference raises, so the oracle is tests/intensity_ref.py, after every step.  width = 20.2 gives an
    odd number of columns: the rows of the uint16 grid then start on odd halfwords, where a counter update wider than 16
    bits would touch its neighbour."""
    settings, geoms, steps, points, logodds = intensity_ref.mapping_session_steps(map_fix)
    m = configured(Mapping(ctx), settings, width=width, **ON)
    ref = ref_map(settings, width=width)
    assert m.cols == ref.cols and (m.cols % 2 == 1) == (width != 20.0)
    shapes = []

    def check(i, st):
        shapes.append((m.rows, m.cols, m.y0, m.x0))

    for i, st in enumerate(steps):          # both step by step, compared after every step
        intensity_ref.replay(m, [st], geoms, points, Pose2, check=check, logodds=logodds)
        intensity_ref.replay(ref, [st], geoms, points, Pose2, logodds=logodds)
        sums_hold(m)
        same_map(m, ref, (i, st["op"], st["key"]))
        assert m.cols % 2 == (1 if width != 20.0 else 0)
    assert np.array_equal(m.logodds_grid.view(np.int32), ref.logodds_grid.view(np.int32))
    assert len({s[2] for s in shapes}) > 1 and len({s[3] for s in shapes}) > 1      # grown on top and on the left ...
    assert max(s[0] for s in shapes) > shapes[0][0] and max(s[1] for s in shapes) > shapes[0][1] + 30   # ... right too
    lc = [s for s, st in zip(shapes, steps) if st.get("pass_") == "lc"]
    assert len(set(lc)) > 1                                                          # growth in the middle of a pose pass
    same_pub(m.get_intensity_grid(), ref.get_intensity_grid())


@pytest.mark.parametrize("values,want", [([6, 6, 6, 6, 6, 7, 7, 7], 2), ([31, 32, 32, 32, 32, 32, 32, 32], 12)])
def test_ties_round_half_to_even(ctx, values, want):
    """eight keyframes at one pose with constant pings that sum to 51 (255): every cell renders 100 * 51 / (255 * 8) = 2.5
    (12.5) exactly, which half-even rounds to 2 (12) and half-up would round to 3 (13)"""
    assert sum(values) in (51, 255) and len(values) == 8
    m = configured(Mapping(ctx), dict(x0=-12.0, y0=-12.0, width=24.0, height=24.0, resolution=0.2), **ON)
    nb, nr, rr = 128, 256, 0.04
    for k, v in enumerate(values):
        m.add_keyframe(k, Pose2(0.5, -0.25, 0.3), mapping_ref.SessionPing(nb, nr, rr), np.zeros((0, 2)),
                       image=np.full((nr, nb), v, np.uint8))
    inten, count = sums_hold(m)
    assert set(np.unique(count)) == {0, 8} and set(np.unique(inten)) == {0, sum(values)}
    msg = m.get_intensity_grid()
    box = (slice(m.rmin, m.rmax + 1), slice(m.cmin, m.cmax + 1))
    assert np.array_equal(msg.occ, np.where(count[box] == 8, want, -1).astype(np.int8)) and (msg.occ == want).sum() > 1000


def test_moving_every_keyframe_and_back_restores_both_grids(ctx, fix, map_fix):
    settings, geoms, steps, points, logodds = intensity_ref.fixture_session(fix, map_fix)
    m = configured(Mapping(ctx), settings, intensity_skips="oculus")
    adds = [st for st in steps if st["op"] == "add"]
    intensity_ref.replay(m, adds, geoms, points, Pose2, logodds=logodds)
    inten, count = sums_hold(m)
    i_before = [kf.i for kf in live(m)]
    grow, shape = list(m._grow), (m.rows, m.cols)
    keys = [st["key"] for st in adds]
    m.update_poses(keys, [Pose2(st["pose"][0] + 0.7, st["pose"][1] - 0.4, st["pose"][2] + 0.2) for st in adds])
    moved = sums_hold(m)
    top, left = m._grow[0] - grow[0], m._grow[1] - grow[1]
    inside = (slice(top, top + shape[0]), slice(left, left + shape[1]))
    assert not np.array_equal(moved[0][inside], inten)
    m.update_poses(keys, [Pose2(*st["pose"]) for st in adds])
    back = sums_hold(m)
    top, left = m._grow[0] - grow[0], m._grow[1] - grow[1]
    inside = (slice(top, top + shape[0]), slice(left, left + shape[1]))
    for got, was in zip(back, (inten, count)):
        assert np.array_equal(got[inside], was) and int(got.sum(dtype=np.int64)) == int(was.sum(dtype=np.int64))
    for a, b in zip(i_before, [kf.i for kf in live(m)]):
        assert np.array_equal(a, b)


def test_mosaic_without_method_1(ctx, fix, map_fix, reference_run):
    """pub_occupancy1=False with the grid on: no measurement is taken, the mosaic is the one built with method 1 on"""
    settings, geoms, steps, points, _ = intensity_ref.fixture_session(fix, map_fix)
    m = configured(Mapping(ctx), settings, intensity_skips="oculus", pub_occupancy1=False)
    intensity_ref.replay(m, steps, geoms, points, Pose2, batched=True)
    sums_hold(m)
    same_map(m, reference_run)
    same_pub(m.get_intensity_grid(), reference_run.get_intensity_grid())


S = 3
SHIFT = [(0.0, 0.0), (1.0, -2.0), (-3.0, 0.5)]


def test_map_batch_sessions_equal_their_own_mappings(ctx, fix, map_fix):
    """three sessions with their own pings (and shifted poses): every maps[s] is, bit for bit, the Mapping given session
    s's calls; a call's apply launches are those of the same call with the grid off"""
    settings, geoms, steps, points, _ = intensity_ref.fixture_session(fix, map_fix)
    adds = [st for st in steps if st["op"] == "add"]
    lc = [st for st in steps if st.get("pass_") == "lc"]
    pose = lambda s, st: Pose2(st["pose"][0] + SHIFT[s][0], st["pose"][1] + SHIFT[s][1], st["pose"][2])

    def run(**over):
        b = MapBatch(ctx, S, 20, max_pixels=8192, **dict(settings, **over))
        b.configure()
        on = bool(over.get("intensity_skips"))
        rounds = []
        for j, st in enumerate(adds):
            nb, nr, rr = geoms[st["geom"]]
            # the last session joins two calls late and so runs on other keys' slots
            sessions = [s for s in range(S) if not (s == 2 and j < 2)]
            images = np.stack([intensity_ref.pattern_ping(st["key"], nr, nb, seed=s) for s in sessions])
            b.add_keyframes(sessions, [st["key"]] * len(sessions), [pose(s, st) for s in sessions],
                            mapping_ref.SessionPing(nb, nr, rr), [np.asarray(points[st["key"]], np.float64)] * len(sessions),
                            **(dict(images=images if j % 2 else list(images)) if on else {}))
            rounds.append(b.last_apply_rounds)
        flat = [(s, st["key"], pose(s, st)) for st in lc for s in range(S) if not (s == 2 and st["key"] < 2)]
        b.update_poses([f[0] for f in flat], [f[1] for f in flat], [f[2] for f in flat])
        rounds.append(b.last_apply_rounds)
        return b, rounds

    b, rounds = run(intensity_skips="oculus")
    off, rounds_off = run(pub_intensity=False)
    assert rounds == rounds_off and rounds[0] == 1 and rounds[-1] >= 2 * len(lc)
    grids = b.get_intensity_grid()
    assert len(grids) == S
    for s in range(S):
        m = configured(Mapping(ctx), settings, intensity_skips="oculus")
        for j, st in enumerate(adds):
            if s == 2 and j < 2:
                continue
            nb, nr, rr = geoms[st["geom"]]
            m.add_keyframe(st["key"], pose(s, st), mapping_ref.SessionPing(nb, nr, rr), np.asarray(points[st["key"]], np.float64),
                           image=intensity_ref.pattern_ping(st["key"], nr, nb, seed=s))
        m.update_poses([st["key"] for st in lc if not (s == 2 and st["key"] < 2)],
                       [pose(s, st) for st in lc if not (s == 2 and st["key"] < 2)])
        sums_hold(b.maps[s])
        same_map(b.maps[s], m, s)
        assert np.array_equal(b.maps[s].logodds_grid.view(np.int32), m.logodds_grid.view(np.int32))
        assert np.array_equal(off.maps[s].logodds_grid.view(np.int32), m.logodds_grid.view(np.int32))
        same_pub(grids[s], m.get_intensity_grid())
        same_pub(b.maps[s].get_intensity_grid(), grids[s])
    assert len(b.get_intensity_grid([2, 0])) == 2
    with pytest.raises(NotImplementedError, match="get_intensity_grid"):
        off.get_intensity_grid()
    b.close()
    off.close()


def test_refusals_leave_the_map_as_it_was(ctx, fix, map_fix):
    settings, geoms, steps, points, _ = intensity_ref.fixture_session(fix, map_fix)
    st = steps[0]
    nb, nr, rr = geoms["A"]
    ping, pts = mapping_ref.SessionPing(nb, nr, rr), np.asarray(points[0], np.float64)
    good = intensity_ref.pattern_ping(0, nr, nb)
    m = configured(Mapping(ctx), settings, intensity_skips="oculus")
    for when in ("first", "second"):
        before = digest(m)
        for bad in (None, good[:-1], good.T, good.astype(np.int16), good[:, ::2]):
            with pytest.raises(ValueError, match="image"):
                m.add_keyframe(len(m.keyframes), Pose2(*st["pose"]), ping, pts, image=bad)
            assert digest(m) == before
        # (a ping of another geometry whose image is misshapen: the geometry is not taken either)
        with pytest.raises(ValueError, match="image"):
            m.add_keyframe(len(m.keyframes), Pose2(*st["pose"]), mapping_ref.SessionPing(*geoms["B"]), pts, image=good)
        assert digest(m) == before
        m.add_keyframe(len(m.keyframes), Pose2(*st["pose"]), ping, pts, image=good)
        assert digest(m) != before
    # image= without the grid
    plain = configured(Mapping(ctx), settings, pub_intensity=False)
    with pytest.raises(ValueError, match="image="):
        plain.add_keyframe(0, Pose2(*st["pose"]), ping, pts, image=good)
    assert plain.keyframes == [] and plain._geom == -1
    # the batch: images= with the grid off, no images= with it on, a slot beyond max_keyframes
    off = MapBatch(ctx, 2, 2, max_pixels=8192, **dict(settings, pub_intensity=False))
    off.configure()
    with pytest.raises(ValueError, match="images="):
        off.add_keyframes([0, 1], [0, 0], [Pose2(*st["pose"])] * 2, ping, [pts, pts], images=[good, good])
    assert off.maps[0].keyframes == [] and off.maps[0]._geom == -1
    b = MapBatch(ctx, 2, 2, max_pixels=8192, **dict(settings, intensity_skips="oculus"))
    b.configure()
    args = lambda k: ([0, 1], [k, k], [Pose2(*st["pose"])] * 2, ping, [pts, pts])
    with pytest.raises(ValueError, match="images="):
        b.add_keyframes(*args(0))
    with pytest.raises(ValueError, match="image"):
        b.add_keyframes(*args(0), images=[good, good[:-1]])
    with pytest.raises(ValueError, match="device image"):
        b.add_keyframes(*args(0), images=[DeviceImage(4096, nr, nb), DeviceImage(4096, nr - 1, nb)])
    assert [digest(v) for v in b.maps] == [digest(v) for v in configured_batch_views(ctx, settings)]
    b.add_keyframes(*args(0), images=[good, good])
    b.add_keyframes(*args(1), images=np.stack([good, good]))
    before = [digest(v) for v in b.maps]
    with pytest.raises(_lib.SonarFEError, match="max_keyframes = 2"):
        b.add_keyframes(*args(2), images=[good, good])
    assert [digest(v) for v in b.maps] == before
    # the device's own checks: an image whose subsampled shape is not the geometry's, a slot beyond the arena
    i32 = lambda *a: np.array(a, np.int32)
    call = lambda slot, rows: b._lib.sfe_mapset_set_intensity(
        b._h, 1, _lib.ptr(i32(0), C.c_int32), _lib.ptr(i32(slot), C.c_int32), _lib.ptr(i32(b.maps[0]._geom), C.c_int32),
        _lib.ptr(i32(rows, nb, 5, 1), C.c_int32), _lib.ptr(np.ascontiguousarray(good), C.c_uint8))
    assert call(1, nr - 5) == _lib.SFE_ERR_ARG and call(2, nr) == _lib.SFE_ERR_CAP
    assert [digest(v) for v in b.maps] == before
    # ... and the grid cannot be switched on once a geometry is registered
    off.add_keyframes([0, 1], [0, 0], [Pose2(*st["pose"])] * 2, ping, [pts, pts])
    assert off._lib.sfe_mapset_enable_intensity(off._h) == _lib.SFE_ERR_ARG
    assert off.maps[0].intensity_grid is None
    b.close()
    off.close()


def configured_batch_views(ctx, settings):
    fresh = MapBatch(ctx, 2, 2, max_pixels=8192, **dict(settings, intensity_skips="oculus"))
    fresh.configure()
    return fresh.maps


def test_session_batch_feeds_the_mosaic_from_its_resident_frames(ctx, shipped_cfar):
    """a batch modelled on tests/test_gpu_slam_cloud.py's with the grid on: every session's grids and rendered image equal a
    Mapping fed the same frames, clouds and poses from the host; the records are those of the batch without the mosaic"""
    from test_global_init import _product_fe, _session
    from test_gpu_map_batch import _same_records
    from sonar_slam_amd import chained, icp_config
    from sonar_slam_amd.feature_extraction import SonarPing, oculus_bearings
    import copy
    K, ROWS, N = 3, 256, 3
    settings = dict(x0=0.0, y0=-20.0, width=40.0, height=40.0, inc=25.0, pub_occupancy2=False)
    sess = [_session(K, rows=ROWS, step=1.7, turn=0.3, seed=21 + 4 * s, n_world=9000, start=(20.0 - 1.5 * s, 0.8 * s, 0.1 * s))
            for s in range(N)]
    frames, dr = np.stack([x[0] for x in sess]), np.stack([x[2] for x in sess])
    ping = SonarPing(frames[0][0], oculus_bearings(frames.shape[-1]), 30.0 / ROWS)

    def batch(**over):
        fe = _product_fe(ctx)
        fe.generate_map_xy(ping)
        sb = chained.SessionBatch(ctx, fe.geometry, shipped_cfar.params["SOCA"], "SOCA", 65, icp_config.shipped_params(), N, K, dr,
                                  ssm_min_points=20, mapping=dict(ping=ping, max_pixels=1 << 16, **dict(settings, **over)))
        for k in range(K):
            sb.upload_frames(k, frames[:, k])
        return sb

    quiet = batch()
    quiet_recs = copy.deepcopy(quiet.run())
    with pytest.raises(NotImplementedError, match="get_intensity_grid"):
        quiet.intensity_grids()
    sb = batch(feed="store", **ON)
    _same_records(copy.deepcopy(sb.run()), quiet_recs)
    grids = sb.intensity_grids()
    assert len(grids) == N and len(sb.intensity_grids([1])) == 1
    for s in range(N):
        m = configured(Mapping(ctx), settings, **ON)
        for k in range(K):
            m.add_keyframe(k, sb._pose(k, s), ping, sb.store.read(sb.handles[s, k]), image=frames[s, k])
        v = sb.maps.maps[s]
        sums_hold(v)
        same_map(v, m, s)
        assert v.counter_grid.max() >= 2 and len(np.unique(v.intensity_grid)) > 50
        assert np.array_equal(v.logodds_grid.view(np.int32), m.logodds_grid.view(np.int32))
        assert np.array_equal(quiet.maps.maps[s].logodds_grid.view(np.int32), m.logodds_grid.view(np.int32))
        same_pub(grids[s], m.get_intensity_grid())
    # the frames must be the map ping's num_ranges x num_bearings
    other = SonarPing(frames[0][0][:-2], oculus_bearings(frames.shape[-1]), 30.0 / ROWS)
    with pytest.raises(ValueError, match="num_ranges x num_bearings"):
        fe = _product_fe(ctx)
        fe.generate_map_xy(ping)
        chained.SessionBatch(ctx, fe.geometry, shipped_cfar.params["SOCA"], "SOCA", 65, icp_config.shipped_params(), N, K, dr,
                             mapping=dict(ping=other, **dict(settings, **ON)))
