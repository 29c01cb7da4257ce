"""The device occupancy map (sonar_slam_amd.mapping, csrc/sfe_map.hip) against the reference's recorded session
(tests/golden/mapping_session.npz, written by the reference's own mapping.py) and against tests/mapping_ref.py."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mapping_ref  # noqa: E402
from mapping_edges import data_agrees, ulps  # noqa: E402
import oracle  # noqa: E402
from sonar_slam_amd import _lib  # noqa: E402
from sonar_slam_amd.mapping import Mapping  # noqa: E402
from sonar_slam_amd.pose2 import Pose2  # noqa: E402

pytestmark = pytest.mark.gpu

FIX = os.path.join(HERE, "golden", "mapping_session.npz")


@pytest.fixture(scope="module")
def fix():
    return np.load(FIX)


@pytest.fixture(scope="module")
def ctx():
    return _lib.default_context()


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def configured(m, fix, **over):
    for k, v in dict(json.loads(str(fix["settings"])), **over).items():
        setattr(m, k, v)
    m.configure()
    return m


def ref_map(fix, **over):
    m = mapping_ref.Mapping()
    m.remove_outlier = oracle.remove_outlier
    return configured(m, fix, **over)


def state(m):
    kfs = [kf for kf in m.keyframes if kf is not None]
    return dict(box=[int(m.rmin), int(m.rmax), int(m.cmin), int(m.cmax)], x0=float(m.x0), y0=float(m.y0), rows=int(m.rows),
                cols=int(m.cols), width=float(m.width), height=float(m.height), grid=sha(m.logodds_grid),
                keyframes=sha(*[a for kf in kfs for a in (kf.r, kf.c, kf.l)]))


@pytest.mark.parametrize("batched", [False, True])
def test_session_from_logodds_is_exact(fix, ctx, batched):
    """fed the reference's log-odds images, every step's box, origin, size, grid bits and r / c / l equal the reference's,
    growth on all four sides included (and growth in the middle of an update_poses batch when batched)"""
    m = configured(Mapping(ctx), fix)
    steps = json.loads(str(fix["steps"]))
    seen = []

    def check(i, st):
        got = state(m)
        for k in ("box", "x0", "y0", "rows", "cols", "width", "height", "grid", "keyframes"):
            assert got[k] == st[k], (i, st["op"], st.get("key"), k, got[k], st[k])
        seen.append(i)
        if st["op"] == "add":
            kf = m.keyframes[st["key"]]
            assert np.array_equal(kf.logodds, fix["logodds_%d" % st["key"]])
        if i + 1 == len(steps) or steps[i + 1]["op"] != st["op"] or steps[i + 1].get("pass_") != st.get("pass_"):
            tag = {"add": "adds"}.get(st["op"], st.get("pass_"))
            if "grid_%s" % tag in fix:
                assert np.array_equal(m.logodds_grid, fix["grid_%s" % tag])
                for j, kf in enumerate(m.keyframes):
                    if kf is not None:
                        for a in "rcl":
                            assert np.array_equal(getattr(kf, a), fix["%s_%s_%d" % (a, tag, j)]), (tag, j, a)

    mapping_ref.replay(m, fix, Pose2, from_logodds=True, batched=batched, check=check)
    assert len(seen) == (len(steps) if not batched else len(seen))
    grows = [(s["rows"], s["cols"], s["y0"], s["x0"]) for s in steps]
    assert len({g[2] for g in grows}) > 1 and len({g[3] for g in grows}) > 1      # grown on top and on the left ...
    assert max(g[0] for g in grows) > grows[0][0] and max(g[1] for g in grows) > grows[0][1]

    # published forms: frames= grid bits equal the reference restatement's; int8 data equal up to near-integer 100 p
    ref = ref_map(fix)
    mapping_ref.replay(ref, fix, Pose2, from_logodds=True)
    assert state(ref) == state(m)
    pubs = json.loads(str(fix["pubs"]))
    for name, kw in pubs.items():
        got = m.get_occupancy_grid(**kw)
        want = ref.get_occupancy_grid1(**kw)
        info = fix["pub_%s_info" % name]
        assert [got.info.origin.position.x, got.info.origin.position.y, got.info.width, got.info.height,
                got.info.resolution] == list(info)
        assert got.header.frame_id == "map" and got.info.origin.orientation.w == 1
        if "frames" in kw:
            assert np.array_equal(m.frames_grid(), ref.last_frames_grid)
        p100 = (100 * want.probs).astype(np.float32)
        data_agrees(got.data, fix["pub_%s_data" % name], p100.ravel())
        assert got.occ.shape == (got.info.height, got.info.width)


def test_session_from_points(fix, ctx):
    """from points: hit masks, first hits and the image before logit bit-equal to mapping_ref; log-odds within 2 ulp;
    r / c exact; published int8 data equal up to near-integer 100 p"""
    m = configured(Mapping(ctx), fix)
    ref = ref_map(fix)
    steps = json.loads(str(fix["steps"]))
    geoms = json.loads(str(fix["geoms"]))
    for st in steps:
        if st["op"] == "add":
            ping = mapping_ref.SessionPing(*geoms[st["geom"]])
            pts = fix["points_%d" % st["key"]].astype(np.float64)
            stages = {}
            ref.add_keyframe(st["key"], Pose2(*st["pose"]), ping, pts, stages=stages)
            m.add_keyframe(st["key"], Pose2(*st["pose"]), ping, pts)
            hits, prob, fh = m.measure_stages()
            if "hits" in stages:
                assert np.array_equal(hits, stages["hits"].astype(np.uint8)), st["key"]
                assert np.array_equal(fh, stages["first_hits"]), st["key"]
            assert np.array_equal(prob.view(np.int32), stages["prob"].view(np.int32)), st["key"]
            kf, rk = m.keyframes[st["key"]], ref.keyframes[st["key"]]
            assert ulps(kf.logodds, rk.logodds).max() <= 2, st["key"]
        else:
            ref.update_pose(st["key"], Pose2(*st["pose"]))
            m.update_pose(st["key"], Pose2(*st["pose"]))
        for kf, rk in zip(m.keyframes, ref.keyframes):
            if kf is not None:
                assert np.array_equal(kf.r, rk.r) and np.array_equal(kf.c, rk.c)
        assert [m.rmin, m.rmax, m.cmin, m.cmax, m.rows, m.cols, m.x0, m.y0] == \
            [ref.rmin, ref.rmax, ref.cmin, ref.cmax, ref.rows, ref.cols, ref.x0, ref.y0]
    assert np.abs(m.logodds_grid - ref.logodds_grid).max() < 1e-4
    for kw in json.loads(str(fix["pubs"])).values():
        got, want = m.get_occupancy_grid(**kw), ref.get_occupancy_grid1(**kw)
        data_agrees(got.data, want.data, (100 * want.probs).astype(np.float32).ravel())


def test_update_poses_equals_update_pose_loop_and_repeats(fix, ctx):
    """update_poses is bit-equal to the update_pose loop (a repeated key included); two runs are bit-identical"""
    def run(batched):
        m = configured(Mapping(ctx), fix)
        mapping_ref.replay(m, fix, Pose2, from_logodds=True, batched=batched)
        keys = [0, 1, 19, 4, 1, 3, 12]
        poses = [Pose2(0.5 * k - 3.0, 0.1 * k, 0.3) for k in keys]
        poses[4] = Pose2(-9.0, 2.0, -1.0)
        if batched:
            m.update_poses(keys, poses)
        else:
            for k, p in zip(keys, poses):
                m.update_pose(k, p)
        return state(m), m.logodds_grid
    a, ga = run(False)
    b, gb = run(True)
    c, gc = run(True)
    assert a == b == c
    assert np.array_equal(ga.view(np.int32), gb.view(np.int32)) and np.array_equal(gb.view(np.int32), gc.view(np.int32))


def test_point_lands_in_its_beam_column(ctx):
    """a return at (rho cos b_j, rho sin b_j) of the keyframe frame is a hit in beam column j"""
    m = Mapping(ctx)
    m.outlier_filter_min_points = 0
    m.configure()
    ping = mapping_ref.SessionPing(256, 512, 0.05)
    bearings = np.deg2rad(np.array(ping.bearings, np.float32) / 100).astype(np.float64)
    for n, (j, rho) in enumerate([(10, 5.0), (128, 12.3), (250, 20.0), (0, 3.3)]):
        pt = np.array([[rho * np.cos(bearings[j]), rho * np.sin(bearings[j])]])
        m.add_keyframe(n, Pose2(0.0, 0.0, 0.0), ping, pt)
        hits, _, _ = m.measure_stages()
        rr, cc = np.nonzero(hits)
        assert list(cc) == [j // m.oculus_c_skip], (j, cc)
        assert list(rr) == [int(round(rho / 0.05 - 1)) // m.oculus_r_skip]


def test_large_geometry_against_mapping_ref(ctx):
    """1024 ranges x 512 beams at 30 m, 200 keyframes and a loop closure that moves them all: grid bits, boxes, origins and
    r / c / l equal mapping_ref's"""
    rng = np.random.default_rng(3)
    ping = mapping_ref.SessionPing(512, 1024, 30.0 / 1024)
    settings = dict(x0=-60.0, y0=-60.0, width=120.0, height=120.0, inc=25.0, resolution=0.2)
    m, ref = Mapping(ctx), mapping_ref.Mapping()
    for obj in (m, ref):
        for k, v in settings.items():
            setattr(obj, k, v)
        obj.configure()
    poses = []
    x = y = th = 0.0
    for k in range(200):
        th += rng.normal(0, 0.08)
        x += 0.8 * np.cos(th)
        y += 0.8 * np.sin(th)
        poses.append((x, y, th))
        if k == 0:
            shape = (171, 512)
        lo = np.where(rng.random(shape) < 0.8, mapping_ref.logit(np.float32(0.3)),
                      rng.uniform(-1, 1.4, shape)).astype(np.float32)
        m.add_keyframe_logodds(k, Pose2(*poses[-1]), ping, lo)
        ref.add_keyframe_logodds(k, Pose2(*poses[-1]), ping, lo)
        if k == 0:
            assert m.oculus_image_size == ref.oculus_image_size == shape
    assert np.array_equal(m.logodds_grid.view(np.int32), ref.logodds_grid.view(np.int32))
    new = [Pose2(px * 1.01 + 1.0, py * 0.99 - 0.5, pth + 0.02) for px, py, pth in poses]
    m.update_poses(list(range(200)), new)
    for k, p in enumerate(new):
        ref.update_pose(k, p)
    assert [m.rmin, m.rmax, m.cmin, m.cmax, m.rows, m.cols, m.x0, m.y0] == \
        [ref.rmin, ref.rmax, ref.cmin, ref.cmax, ref.rows, ref.cols, ref.x0, ref.y0]
    assert np.array_equal(m.logodds_grid.view(np.int32), ref.logodds_grid.view(np.int32))
    for k in (0, 57, 123, 199):
        for a in "rcl":
            assert np.array_equal(getattr(m.keyframes[k], a), getattr(ref.keyframes[k], a)), (k, a)
