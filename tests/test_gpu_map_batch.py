"""mapping.MapBatch (csrc/sfe_map.hip: sfe_mapset): S occupancy maps in lock-step.  The references are the one-map
``Mapping``, tests/mapping_ref.py and the reference's recorded session (tests/golden/mapping_session.npz) -- never MapBatch
against itself: every session of a batch must be, bit for bit, the Mapping that was given that session's calls."""
import json
import os
import re
import sys
import types

import ctypes as C
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import mapping_ref  # noqa: E402
from test_map_batch_host import apply_rounds  # noqa: E402
from test_gpu_mapping import configured, data_agrees, ref_map, sha, state, ulps  # noqa: E402
from sonar_slam_amd import _lib  # noqa: E402
from sonar_slam_amd import mapping  # noqa: E402
from sonar_slam_amd.mapping import MapBatch, Mapping  # noqa: E402
from sonar_slam_amd.pose2 import Pose2  # noqa: E402

pytestmark = pytest.mark.gpu

FIX = os.path.join(HERE, "golden", "mapping_session.npz")
S = 4
# session s replays the recorded session with its poses rotated by MOVES[s][0] about the origin and shifted by MOVES[s][1:]
MOVES = [(0.0, 0.0, 0.0), (0.7, 3.0, -4.0), (2.0, -5.0, 2.0), (-1.3, 1.0, 6.0)]
PIXELS = {"A": 6656, "B": 8192}
LAG = 2                     # session 3 runs two add calls behind: absent from the first two, alone in the last two
DROPPED = {1: 7}            # session 1 misses key 7 as well as the fixture's key 3


@pytest.fixture(scope="module")
def fix():
    return np.load(FIX)


def moved(s, pose):
    a, dx, dy = MOVES[s]
    if s == 0:
        return Pose2(*pose)
    x, y, th = pose
    return Pose2(np.cos(a) * x - np.sin(a) * y + dx, np.sin(a) * x + np.cos(a) * y + dy, th + a)


def geom_of(s, st):
    """session 2 changes geometry at key 2 instead of key 6"""
    return "B" if s == 2 and 2 <= st["key"] < 6 else st["geom"]


def data_of(fix, s, st, from_logodds):
    if not from_logodds:
        return fix["points_%d" % st["key"]].astype(np.float64)
    if geom_of(s, st) == st["geom"]:
        return fix["logodds_%d" % st["key"]]
    rng = np.random.default_rng(100 * s + st["key"])
    n = PIXELS[geom_of(s, st)]
    return np.where(rng.random(n) < 0.8, mapping_ref.logit(np.float32(0.3)), rng.uniform(-1, 1.4, n)).astype(np.float32)


def add_calls(fix, from_logodds):
    """-> [call][(session, fixture step index, key, pose, ping, data)]"""
    geoms = json.loads(str(fix["geoms"]))
    adds = [(i, st) for i, st in enumerate(json.loads(str(fix["steps"]))) if st["op"] == "add"]
    calls = []
    for j in range(len(adds) + LAG):
        call = []
        for s in range(S):
            jj = j - LAG if s == 3 else j
            if not 0 <= jj < len(adds):
                continue
            i, st = adds[jj]
            if DROPPED.get(s) == st["key"]:
                continue
            call.append((s, i, st["key"], moved(s, st["pose"]), mapping_ref.SessionPing(*geoms[geom_of(s, st)]),
                         data_of(fix, s, st, from_logodds)))
        calls.append(call)
    return calls


def pose_pass(fix, names):
    """-> flat (sessions, keys, poses) of the named pose passes, the sessions interleaved"""
    steps = [st for st in json.loads(str(fix["steps"])) if st["op"] == "update" and st["pass_"] in names]
    flat = [(s, st["key"], moved(s, st["pose"])) for st in steps for s in range(S)]
    return [f[0] for f in flat], [f[1] for f in flat], [f[2] for f in flat]


def new_batch(ctx, fix, max_keyframes=20, **over):
    b = MapBatch(ctx, S, max_keyframes, max_pixels=8192, **dict(json.loads(str(fix["settings"])), **over))
    b.configure()
    return b


def singles(ctx, fix, **over):
    return [configured(Mapping(ctx), fix, **over) for _ in range(S)]


def add_all(fix, b, ms, from_logodds, after=None):
    for j, call in enumerate(add_calls(fix, from_logodds)):
        args = [[c[k] for c in call] for k in (0, 2, 3, 4, 5)]
        if b is not None:
            (b.add_keyframes_logodds if from_logodds else b.add_keyframes)(*args)
        for s, i, key, pose, ping, data in call:
            if ms is not None:
                (ms[s].add_keyframe_logodds if from_logodds else ms[s].add_keyframe)(key, pose, ping, data)
            after and after(s, i, key)


def device_shape(m):
    out = np.zeros(4, np.int32)
    m._check(m._lib.sfe_map_shape(m._h, _lib.ptr(out, C.c_int32)))
    return tuple(int(v) for v in out)


def same(v, m, tag="", same_calls=True):
    """a MapBatch session against a Mapping: every bit of the state.  `same_calls`: the Mapping was given the same calls, so
    even the bookkeeping of when a cell list was written (its box and the growth counters then) is equal; against the
    update_pose loop only the box in the grid's current coordinates is, because a loop writes each list before the growth that
    later keyframes of the same pass cause."""
    assert state(v) == state(m), tag
    assert np.array_equal(v.logodds_grid.view(np.int32), m.logodds_grid.view(np.int32)), tag
    assert v.device_shape() == device_shape(m) == (m.rows, m.cols, m._grow[0], m._grow[1]), tag
    assert v._grow == m._grow and len(v.keyframes) == len(m.keyframes), tag
    assert (v.oculus_image_size, v.oculus_r_skip, v.oculus_c_skip) == (m.oculus_image_size, m.oculus_r_skip, m.oculus_c_skip)
    for k, (a, b) in enumerate(zip(v.keyframes, m.keyframes)):
        assert (a is None) == (b is None), (tag, k)
        if a is None:
            continue
        assert (a.k, a.cell_box()) == (b.k, b.cell_box()), (tag, k)
        if same_calls:
            assert (a.box, a.base) == (b.box, b.base), (tag, k)
        assert (a.pose.x(), a.pose.y(), a.pose.theta()) == (b.pose.x(), b.pose.y(), b.pose.theta()), (tag, k)
        for name in ("r", "c", "l", "logodds"):
            x, y = getattr(a, name), getattr(b, name)
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (tag, k, name)


def digest(b):
    return [(state(v), v.device_shape(), sha(*[kf.logodds for kf in v.keyframes if kf is not None]), len(v.keyframes),
             v._n_slots, v.oculus_image_size, v.oculus_r_skip, v.oculus_c_skip, v._geom, sorted(v._geom_shape.items()),
             sha(*[np.asarray(x) for x in (v.oculus.num_ranges or 0, v.oculus.range_resolution or 0.0,
                                           v.oculus.num_bearings or 0, v.oculus.max_range)]),
             None if v.oculus.bearings is None else sha(v.oculus.bearings, v.oculus.ranges)) for v in b.maps]


def test_recorded_session_from_logodds_inside_a_batch(fix, ctx):
    """session 0 = the reference's recorded session, step by step (box, origin, size, grid sha, r / c / l); sessions 1-3 the
    same session rotated and shifted (other growth steps and sides), one missing another key, one changing geometry at another
    step, one absent from calls: all four bit-equal to independent Mappings"""
    b, ms = new_batch(ctx, fix), singles(ctx, fix)
    steps = json.loads(str(fix["steps"]))
    seen = []

    def after(s, i, key):
        if s:
            return
        got, st = state(b.maps[0]), steps[i]
        for k in ("box", "x0", "y0", "rows", "cols", "width", "height", "grid", "keyframes"):
            assert got[k] == st[k], (i, key, k, got[k], st[k])
        assert np.array_equal(b.maps[0].keyframes[key].logodds, fix["logodds_%d" % key])
        seen.append(i)

    add_all(fix, b, ms, True, after)
    assert len(seen) == 19
    assert np.array_equal(b.maps[0].logodds_grid, fix["grid_adds"])
    for j, kf in enumerate(b.maps[0].keyframes):
        if kf is not None:
            for a in "rcl":
                assert np.array_equal(getattr(kf, a), fix["%s_adds_%d" % (a, j)]), (j, a)
    for s in range(S):
        same(b.maps[s], ms[s], "session %d" % s)
    # the sessions really differ from each other: growth on other sides, other keys, other geometries
    assert len({(v.x0, v.y0, v.rows, v.cols) for v in b.maps}) > 1
    assert b.maps[1].keyframes[7] is None and b.maps[0].keyframes[7] is not None
    assert b.maps[2].keyframes[4].geom != b.maps[0].keyframes[4].geom
    assert len(b._geoms) == 2                                        # equal sonar_xy tables are stored once


def test_recorded_session_from_points_inside_a_batch(fix, ctx):
    """from points, session 0 under test_session_from_points' rules against mapping_ref (hit masks, first hits and the image
    before logit bit-equal, log-odds within 2 ulp, r / c exact); every session bit-equal to its own Mapping"""
    b, ms = new_batch(ctx, fix), singles(ctx, fix)
    ref = ref_map(fix)
    steps = json.loads(str(fix["steps"]))
    geoms = json.loads(str(fix["geoms"]))

    def after(s, i, key):
        if s:
            return
        st, v = steps[i], b.maps[0]
        stages = {}
        ref.add_keyframe(key, Pose2(*st["pose"]), mapping_ref.SessionPing(*geoms[st["geom"]]),
                         fix["points_%d" % key].astype(np.float64), stages=stages)
        hits, prob, fh = v.measure_stages()
        if "hits" in stages:
            assert np.array_equal(hits, stages["hits"].astype(np.uint8)), key
            assert np.array_equal(fh, stages["first_hits"]), key
        assert np.array_equal(prob.view(np.int32), stages["prob"].view(np.int32)), key
        assert ulps(v.keyframes[key].logodds, ref.keyframes[key].logodds).max() <= 2, key
        for kf, rk in zip(v.keyframes, ref.keyframes):
            if kf is not None:
                assert np.array_equal(kf.r, rk.r) and np.array_equal(kf.c, rk.c)
        assert [v.rmin, v.rmax, v.cmin, v.cmax, v.rows, v.cols, v.x0, v.y0] == \
            [ref.rmin, ref.rmax, ref.cmin, ref.cmax, ref.rows, ref.cols, ref.x0, ref.y0]

    add_all(fix, b, ms, False, after)
    for s in range(S):
        same(b.maps[s], ms[s], "session %d" % s)
    sessions, keys, poses = pose_pass(fix, ("lc", "nudge", "missed"))
    b.update_poses(sessions, keys, poses)
    for st in steps:
        if st["op"] == "update":
            ref.update_pose(st["key"], Pose2(*st["pose"]))
    v = b.maps[0]
    for kf, rk in zip(v.keyframes, ref.keyframes):
        if kf is not None:
            assert np.array_equal(kf.r, rk.r) and np.array_equal(kf.c, rk.c)
    assert np.abs(v.logodds_grid - ref.logodds_grid).max() < 1e-4
    pubs = json.loads(str(fix["pubs"]))
    for kw in pubs.values():
        got, want = b.get_occupancy_grids([0], **kw)[0], ref.get_occupancy_grid1(**kw)
        data_agrees(got.data, want.data, (100 * want.probs).astype(np.float32).ravel())


def test_loop_closure_across_sessions_and_published_forms(fix, ctx):
    """one update_poses call with the fixture's lc and nudge passes of all four sessions (growth in the middle of the pass,
    every nudged key listed twice) = per-session Mapping.update_poses = the update_pose loop; session 0 ends on the
    reference's recorded grid.  Then every published form of every session against its own Mapping's."""
    b, ms, loops = new_batch(ctx, fix), singles(ctx, fix), singles(ctx, fix)
    add_all(fix, b, ms, True)
    add_all(fix, None, loops, True)
    rows_before = [v.rows for v in b.maps]
    sessions, keys, poses = pose_pass(fix, ("lc", "nudge", "missed"))
    assert len(keys) > len(set(zip(sessions, keys)))                 # keys listed twice
    # the launches the schedule allows, from the planner on copies of the keyframes' poses: rounds, not 2 * (sessions x keyframes)
    copies = [[kf and types.SimpleNamespace(k=kf.k, pose=kf.pose) for kf in v.keyframes] for v in b.maps]
    waves = mapping.plan_updates(copies, [v.pose_changed for v in b.maps], sessions, keys, poses)
    want_rounds = sum(len(apply_rounds(w, dec=True)) for w in waves)
    n_refits = sum(len(g) for w in waves for _, g in w)
    assert len(waves) == 2 and 2 * 19 <= want_rounds <= 2 * (19 + 8) and n_refits > 3 * 19
    b.update_poses(sessions, keys, poses)
    assert b.last_apply_rounds == want_rounds                        # counted by the device code, launch by launch
    for s in range(S):
        mine = [(k, p) for ss, k, p in zip(sessions, keys, poses) if ss == s]
        ms[s].update_poses([k for k, _ in mine], [p for _, p in mine])
        for k, p in mine:
            loops[s].update_pose(k, p)
        same(b.maps[s], ms[s], "update_poses, session %d" % s)
        same(b.maps[s], loops[s], "update_pose loop, session %d" % s, same_calls=False)
    assert b.maps[0].rows > rows_before[0]                           # growth in the middle of the pass
    assert np.array_equal(b.maps[0].logodds_grid, fix["grid_nudge"])
    for j, kf in enumerate(b.maps[0].keyframes):
        if kf is not None:
            for a in "rcl":
                assert np.array_equal(getattr(kf, a), fix["%s_nudge_%d" % (a, j)]), (j, a)
    final = json.loads(str(fix["steps"]))[-1]
    got = state(b.maps[0])
    for k in ("box", "x0", "y0", "rows", "cols", "width", "height", "grid", "keyframes"):
        assert got[k] == final[k], k

    # published forms
    pubs = json.loads(str(fix["pubs"]))
    for name, kw in pubs.items():
        msgs = b.get_occupancy_grids(**kw)
        assert len(msgs) == S
        for s in range(S):
            got, want = msgs[s], ms[s].get_occupancy_grid(**kw)
            assert np.array_equal(got.occ, want.occ) and got.occ.dtype == np.int8, (name, s)
            assert list(got.data) == list(want.data), (name, s)
            assert vars(got.info.origin.position) == vars(want.info.origin.position), (name, s)
            assert vars(got.info.origin.orientation) == vars(want.info.origin.orientation), (name, s)
            assert (got.info.width, got.info.height, got.info.resolution, got.header.frame_id) == \
                (want.info.width, want.info.height, want.info.resolution, want.header.frame_id), (name, s)
            if "frames" in kw:
                assert np.array_equal(b.maps[s].frames_grid().view(np.int32), ms[s].frames_grid().view(np.int32)), (name, s)
        info = fix["pub_%s_info" % name]
        g0 = msgs[0]
        assert [g0.info.origin.position.x, g0.info.origin.position.y, g0.info.width, g0.info.height,
                g0.info.resolution] == list(info)
    # a subset of the sessions, in another order, and one session through its view
    kw = pubs["frames_coarse"]
    sub = b.get_occupancy_grids([3, 1], **kw)
    for got, s in zip(sub, (3, 1)):
        assert np.array_equal(got.occ, ms[s].get_occupancy_grid(**kw).occ)
    assert np.array_equal(b.maps[2].get_occupancy_grid(**kw).occ, ms[2].get_occupancy_grid(**kw).occ)


def test_capacity_is_refused_loudly_and_changes_nothing(fix, ctx):
    """one keyframe beyond max_keyframes raises before anything changes; so does an image larger than max_pixels"""
    b = new_batch(ctx, fix, max_keyframes=3)
    calls = add_calls(fix, True)
    for call in calls[:2]:
        call = [c for c in call if c[0] in (0, 1)]
        b.add_keyframes_logodds(*[[c[k] for c in call] for k in (0, 2, 3, 4, 5)])
    only1 = [c for c in calls[2] if c[0] == 1]
    b.add_keyframes_logodds(*[[c[k] for c in only1] for k in (0, 2, 3, 4, 5)])       # session 1 is full, session 0 is not
    before = digest(b)
    both = [c for c in calls[3] if c[0] in (0, 1)]
    with pytest.raises(_lib.SonarFEError, match="max_keyframes = 3"):
        b.add_keyframes_logodds(*[[c[k] for c in both] for k in (0, 2, 3, 4, 5)])
    assert digest(b) == before
    pts = [c for c in add_calls(fix, False)[3] if c[0] in (0, 1)]
    with pytest.raises(_lib.SonarFEError, match="max_keyframes = 3"):
        b.add_keyframes(*[[c[k] for c in pts] for k in (0, 2, 3, 4, 5)])
    assert digest(b) == before
    # the session with room still takes its keyframe, and is the Mapping given the same three calls
    zero = [c for c in calls[2] if c[0] == 0]
    b.add_keyframes_logodds(*[[c[k] for c in zero] for k in (0, 2, 3, 4, 5)])
    m = configured(Mapping(ctx), fix)
    for call in calls[:3]:
        for s, i, key, pose, ping, data in call:
            if s == 0:
                m.add_keyframe_logodds(key, pose, ping, data)
    same(b.maps[0], m)
    # the device refuses on its own, too: a slot beyond the arena, an image beyond max_pixels
    i32 = lambda *a: _lib.ptr(np.array(a, np.int32), C.c_int32)
    lo = np.zeros(8192, np.float32)
    assert b._lib.sfe_mapset_set_logodds(b._h, 1, i32(0), i32(3), i32(0), _lib.ptr(lo, C.c_float)) == _lib.SFE_ERR_CAP
    small = MapBatch(ctx, 2, 3, max_pixels=6000, **json.loads(str(fix["settings"])))
    small.configure()
    s, i, key, pose, ping, data = calls[0][0]
    # ... at the first keyframe of all: nothing changes, and the next call is refused the same way, not run with a stale geometry
    for _ in range(2):
        before = digest(small)
        with pytest.raises(_lib.SonarFEError, match="room for 6000 pixels"):
            small.add_keyframes_logodds([0, 1], [key, key], [pose, pose], ping, [data, data])
        assert digest(small) == before and small.maps[0]._geom == -1
    # ... and after a geometry that fits: the refusal leaves every session's sonar state as it was, a following ping of the
    # first geometry is added as a Mapping adds it, and the refused geometry is refused again from points too
    geoms = json.loads(str(fix["geoms"]))
    big = mapping_ref.SessionPing(*geoms["B"])                       # 8192 pixels
    room = MapBatch(ctx, 2, 3, max_pixels=7000, **json.loads(str(fix["settings"])))
    room.configure()
    m = configured(Mapping(ctx), fix)
    lo_a = fix["logodds_0"]
    room.add_keyframes_logodds([0, 1], [0, 0], [pose, pose], ping, [lo_a, lo_a])       # geometry A: 6656 pixels
    m.add_keyframe_logodds(0, pose, ping, lo_a)
    before = digest(room)
    with pytest.raises(_lib.SonarFEError, match="room for 7000 pixels"):
        room.add_keyframes_logodds([0, 1], [1, 1], [pose, pose], big, [np.zeros(8192, np.float32)] * 2)
    assert digest(room) == before
    pts = fix["points_1"].astype(np.float64)
    with pytest.raises(_lib.SonarFEError, match="room for 7000 pixels"):
        room.add_keyframes([1, 0], [1, 1], [pose, pose], big, [pts, pts])
    assert digest(room) == before
    pose1 = Pose2(2.0, 0.5, 0.1)
    room.add_keyframes_logodds([0], [1], [pose1], ping, [fix["logodds_1"]])
    room.add_keyframes([1], [1], [pose1], ping, [pts])
    m.add_keyframe_logodds(1, pose1, ping, fix["logodds_1"])
    same(room.maps[0], m, "after the refused geometry")
    m2 = configured(Mapping(ctx), fix)
    m2.add_keyframe_logodds(0, pose, ping, lo_a)
    m2.add_keyframe(1, pose1, ping, pts)
    same(room.maps[1], m2, "after the refused geometry, from points")
    with pytest.raises(ValueError, match="listed twice"):
        b.add_keyframes_logodds([0, 0], [9, 9], [pose, pose], ping, [data, data])


def _same_records(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert set(x) == set(y)
        for k in x:
            if isinstance(x[k], np.ndarray):
                assert x[k].dtype == y[k].dtype and np.array_equal(x[k], y[k], equal_nan=x[k].dtype.kind == "f"), k
            else:
                assert x[k] == y[k], k


def test_session_batch_feeds_its_maps(ctx, shipped_cfar):
    """SessionBatch(mapping=...): records and loops as without it; every session's map = a Mapping fed the store's clouds and
    the recorded poses; reset() and a second run give the same maps"""
    import copy
    from test_global_init import _product_fe, _session
    from sonar_slam_amd import chained, icp_config
    from sonar_slam_amd.feature_extraction import SonarPing, oculus_bearings
    K, ROWS, n = 5, 256, 3
    sess = [_session(K, rows=ROWS, step=1.7, turn=0.3, seed=21 + 4 * s, n_world=9000, start=(20.0 - 1.5 * s, 0.8 * s, 0.1 * s))
            for s in range(n)]
    pings, dr = np.stack([x[0] for x in sess]), np.stack([x[2] for x in sess])
    ping = SonarPing(pings[0][0], oculus_bearings(pings.shape[-1]), 30.0 / ROWS)
    settings = dict(x0=0.0, y0=-20.0, width=40.0, height=40.0, inc=25.0)

    def batch(**kw):
        fe = _product_fe(ctx)
        fe.generate_map_xy(ping)
        sb = chained.SessionBatch(ctx, fe.geometry, shipped_cfar.params["SOCA"], "SOCA", 65, icp_config.shipped_params(), n, K, dr,
                                  ssm_min_points=20, **kw)
        for k in range(K):
            sb.upload_frames(k, pings[:, k])
        return sb

    plain = batch()
    assert plain.maps is None
    want_recs, want_loops = copy.deepcopy(plain.run()), copy.deepcopy(plain.loops)
    plain.free()
    sb = batch(mapping=dict(ping=ping, max_pixels=1 << 16, **settings))
    recs = copy.deepcopy(sb.run())
    _same_records(recs, want_recs)
    assert sb.loops == want_loops
    assert len(sb.store) == n * K
    first = digest(sb.maps)
    grew = 0
    for s in range(n):
        m = Mapping(ctx)
        for k, v in settings.items():
            setattr(m, k, v)
        m.configure()
        for k in range(K):
            m.add_keyframe(k, sb._pose(k, s), ping, sb.store.read(sb.handles[s, k]))
            assert tuple(recs[k]["pose"][s][:2]) == (m.keyframes[k].pose.x(), m.keyframes[k].pose.y())
        same(sb.maps.maps[s], m, "session %d" % s)
        assert len(m.keyframes) == K and np.count_nonzero(m.logodds_grid) > 1000
        grew += m.rows > 200 or m.cols > 200
    assert grew
    sb.reset()
    assert all(v.keyframes == [] for v in sb.maps.maps)
    _same_records(copy.deepcopy(sb.run()), want_recs)
    assert digest(sb.maps) == first
    sb.free()


def test_sources_keep_to_the_machine_rules():
    """the sources of the map set hold no scalar store or scalar atomic mnemonic, no hardware-queue setting above 32 and no
    graph-replay override"""
    # (the patterns are put together from pieces, so that this file passes its own scan)
    scalar = "s" + "_"
    banned = re.compile("|".join([scalar + "(buffer_|scratch_)?" + "store_", scalar + "(buffer_)?" + "atomic_",
                                  scalar + "dcache" + "_(wb|discard)", "FORCE_" + "GRAPH_" + "QUEUES"]), re.I)
    files = ["sonar_slam_amd/csrc/sfe_map.hip", "sonar_slam_amd/csrc/sfe_store.hip", "sonar_slam_amd/mapping.py",
             "sonar_slam_amd/chained.py", "sonar_slam_amd/store.py", "include/sonarfe.h", "tools/mapping_times.py",
             "tests/test_gpu_map_batch.py", "tests/test_map_batch_host.py"]
    for f in files:
        txt = open(os.path.join(ROOT, f)).read()
        assert not banned.search(txt), f
        for q in re.findall(r"GPU_MAX_HW_QUEUES\D{0,4}(\d+)", txt):
            assert int(q) <= 32, f
