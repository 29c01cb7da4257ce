"""Method 2 (get_occupancy_grid2: sfe_map_render2 / sfe_mapset_render2 in csrc/sfe_map.hip) on the device, bit for bit
against the reference's recorded publications (tests/golden/mapping2_session.npz, written by the reference's own
mapping.py) and against the numpy restatement tests/mapping2_ref.py at the shapes where the kernels can go wrong."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mapping2_ref  # noqa: E402
import mapping_ref  # noqa: E402
import oracle  # noqa: E402
from sonar_slam_amd import _lib  # noqa: E402
from sonar_slam_amd.mapping import MapBatch, Mapping  # noqa: E402
from sonar_slam_amd.pose2 import Pose2  # noqa: E402

pytestmark = pytest.mark.gpu

SETTINGS = dict(x0=-10.0, y0=-10.0, width=20.0, height=20.0, inc=6.0, resolution=0.2, outlier_filter_radius=2.0,
                outlier_filter_min_points=8, min_translation=0.5, min_rotation=0.05)
PINGS = {"A": mapping_ref.SessionPing(128, 256, 0.04), "B": mapping_ref.SessionPing(256, 128, 0.08)}
# the first two keyframes fit the 20 m map; the later ones leave it on the left and on top (y0 falls), so the first cell
# lists are read shifted; key 3 is missed
HISTORY = [(0, "A", (0.0, 0.0, 0.0)), (1, "B", (2.0, 1.0, 0.4)), (2, "A", (-4.0, 0.0, 3.1)), (4, "A", (-1.0, -4.0, -1.6)),
           (5, "B", (3.0, 3.0, 1.2))]


@pytest.fixture(scope="module")
def ctx():
    return _lib.default_context()


def info_of(msg):
    return [msg.info.origin.position.x, msg.info.origin.position.y, msg.info.width, msg.info.height, msg.info.resolution]


def fan_points(rng, n, max_range):
    b, rho = rng.uniform(-1.0, 1.0, n), rng.uniform(0.5, 0.95 * max_range, n)
    return np.c_[rho * np.cos(b), rho * np.sin(b)].astype(np.float32).astype(np.float64)


def registered(points, pose, key):
    """a keyframe's points in the map frame: float32 x, y, 0, key"""
    x, y, th = pose
    c, s = np.cos(th), np.sin(th)
    g = np.c_[c * points[:, 0] - s * points[:, 1] + x, s * points[:, 0] + c * points[:, 1] + y]
    return np.c_[g, np.zeros(len(g)), np.full(len(g), float(key))].astype(np.float32)


def history_clouds(history, seed):
    rng = np.random.default_rng(seed)
    local = [fan_points(rng, 60, 10.0) for _ in history]
    return local, np.concatenate([registered(p, pose, key) for p, (key, _, pose) in zip(local, history)])


def new_map(ctx, history=HISTORY, seed=3, **over):
    m = Mapping(ctx)
    for k, v in dict(SETTINGS, **over).items():
        setattr(m, k, v)
    m.configure()
    local, cloud = history_clouds(history, seed)
    for (key, geom, pose), pts in zip(history, local):
        m.add_keyframe(key, Pose2(*pose), PINGS[geom], cloud if not m.pub_occupancy1 else pts)
    return m, cloud


def cells_of(m):
    return [None if kf is None else (kf.r, kf.c) for kf in m.keyframes]


def expect(m, cells, cloud, **kw):
    return mapping2_ref.occupancy_grid2(m, cells, cloud, oracle.remove_outlier, **kw)


def agree(msg, want, tag=None):
    assert info_of(msg) == list(want["info"]), tag
    assert msg.occ.dtype == np.int8 and msg.occ.shape == want["data"].shape, tag
    assert np.array_equal(msg.occ, want["data"]), (tag, np.argwhere(msg.occ != want["data"])[:8])
    assert msg.data == list(want["data"].ravel()), tag


# ---- the reference's session ------------------------------------------------------------------------------------------------
def test_session_publications_equal_the_reference(ctx):
    """every publication of both stages: data bit for bit, info and the known region's box; frames=[3, 99] marks nothing"""
    first = np.load(os.path.join(HERE, "golden", "mapping_session.npz"))
    fix = np.load(os.path.join(HERE, "golden", "mapping2_session.npz"))
    pubs = json.loads(str(fix["pubs"]))
    steps = json.loads(str(first["steps"]))
    ends = {max(i for i, s in enumerate(steps) if s["op"] == "add"): "adds",
            max(i for i, s in enumerate(steps) if s.get("pass_") == "lc"): "lc"}
    m = Mapping(ctx)
    for k, v in json.loads(str(fix["settings"])).items():
        setattr(m, k, v)
    m.configure()
    keep = dict(outlier_filter_min_points=m.outlier_filter_min_points, dilate_size=m.dilate_size)
    assert m.dilate_size == int(fix["dilate_size"])
    done = []

    def check(i, st):
        stage = ends.get(i)
        if stage is None:
            return
        for name, (kw, which, over) in pubs.items():
            for k, v in dict(keep, **over).items():
                setattr(m, k, v)
            m.point_cloud = np.zeros((0, 4), np.float32) if which == "empty" else fix["%s_%s" % (which, stage)]
            tag = "pub_%s_%s_" % (stage, name)
            msg = m.get_occupancy_grid2(**kw)
            assert list(m._render2_plan(kw.get("frames"), kw.get("resolution"))[1]) == list(fix[tag + "box"]), tag
            assert info_of(msg) == list(fix[tag + "info"]), tag
            got, want = msg.occ.ravel(), fix[tag + "data"]
            assert got.shape == want.shape and np.array_equal(got, want), (tag, int((got != want).sum()))
            assert msg.header.frame_id == "map" and msg.info.origin.orientation.w == 1
        for k, v in keep.items():
            setattr(m, k, v)
        with pytest.raises(IndexError):
            m.get_occupancy_grid2(frames=[3, 99])
        done.append(stage)

    mapping_ref.replay(m, first, Pose2, check=check)
    assert done == ["adds", "lc"]


# ---- small shapes against the restatement -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grown(ctx):
    """a map grown on top and on the left after its first keyframes were written, and their cell lists"""
    m, cloud = new_map(ctx)
    assert m._grow[0] > 0 and m._grow[1] > 0 and m.keyframes[0].base == (0, 0) and m.keyframes[3] is None
    return m, cloud, cells_of(m)


def region(m, frames=None):
    _, (rmin, rmax, cmin, cmax), (y0, x0), _, _, _, _ = m._render2_plan(frames, None)
    return y0, x0, rmax - rmin + 1, cmax - cmin + 1


def at_cells(m, rc, frames=None):
    """float64 points at the centres of region cells (row, column)"""
    y0, x0, _, _ = region(m, frames)
    rc = np.asarray(rc, np.float64)
    return np.c_[x0 + rc[:, 1] * m.resolution, y0 + rc[:, 0] * m.resolution]


def corner_points(m):
    _, _, h, w = region(m)
    return at_cells(m, [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)])


def outside_points(m):
    _, _, h, w = region(m)
    return at_cells(m, [(-1, 5), (h, 7), (9, -1), (11, w), (-1, -1), (h, w), (h // 2, w // 2)])


def big_cloud(m):
    """2305 points: past one 2048-point tile of the filter, not a multiple of 256; clusters the filter keeps, strays it drops"""
    rng = np.random.default_rng(11)
    y0, x0, h, w = region(m)
    centres = np.c_[rng.uniform(x0, x0 + w * m.resolution, 45), rng.uniform(y0, y0 + h * m.resolution, 45)]
    pts = np.concatenate([centres.repeat(50, axis=0) + rng.normal(0.0, 0.4, (2250, 2)),
                          np.c_[rng.uniform(x0 - 3, x0 + w * m.resolution + 3, 55), rng.uniform(y0 - 3, y0 + h * m.resolution + 3, 55)]])
    assert len(pts) == 2305
    return pts


CASES = {
    # name: (cloud builder, settings changed, get_occupancy_grid2's arguments)
    "2305_points": (big_cloud, dict(outlier_filter_radius=0.8, outlier_filter_min_points=12), dict()),
    "2305_points_float32_resized": (lambda m: big_cloud(m).astype(np.float32), dict(outlier_filter_radius=0.8,
                                                                                 outlier_filter_min_points=12), dict(resolution=0.5)),
    "corners": (corner_points, dict(outlier_filter_min_points=1), dict()),
    "corners_wide_element": (corner_points, dict(outlier_filter_min_points=1, dilate_size=11), dict()),
    "dilate_size_1": (lambda m: np.r_[corner_points(m), at_cells(m, [(3, 4), (3, 5), (40, 2)])],
                      dict(outlier_filter_min_points=1, dilate_size=1), dict()),
    "one_cell_outside": (outside_points, dict(outlier_filter_min_points=1), dict()),
    "one_cell_outside_filtered": (lambda m: outside_points(m).repeat(3, axis=0), dict(outlier_filter_min_points=2,
                                                                                      outlier_filter_radius=0.01), dict()),
    "n_by_3": (lambda m: np.c_[big_cloud(m)[:300], np.zeros(300)], dict(), dict(resolution=0.45)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_small_shapes_equal_the_restatement(grown, name):
    m, _, cells = grown
    build, over, kw = CASES[name]
    keep = {k: getattr(m, k) for k in over}
    try:
        for k, v in over.items():
            setattr(m, k, v)
        m.point_cloud = build(m)
        want = expect(m, cells, m.point_cloud, **kw)
        got = m.get_occupancy_grid2(**kw)
    finally:
        for k, v in keep.items():
            setattr(m, k, v)
    agree(got, want, name)
    assert (want["data"] == 100).any() and (want["data"] == 0).any() and (want["data"] == -1).any()
    if name.startswith("2305"):
        assert 0 < want["kept"] < 2305
    if name.startswith("one_cell_outside"):
        assert (want["data"] == 100).sum() == mapping2_ref.ellipse_element(m.dilate_size).sum()      # the one point inside
    if name == "corners":
        assert all(want["data"][r, c] == 100 for r in (0, -1) for c in (0, -1))


def test_keyed_cloud_frames_on_a_grown_map(grown):
    """the N x 4 cloud the adds build: all of it, and by frames (a duplicate, the missed key, a key out of range)"""
    m, cloud, cells = grown
    m.point_cloud = cloud
    for kw in (dict(), dict(frames=[4, 0, 3, 77, 0]), dict(frames=[1, 5], resolution=0.5)):
        agree(m.get_occupancy_grid2(**kw), expect(m, cells, cloud, **kw), kw)
    with pytest.raises(IndexError):
        m.get_occupancy_grid2(frames=[3, 99])
    with pytest.raises(IndexError):                 # frames= reads column 3
        m.point_cloud = cloud[:, :2]
        m.get_occupancy_grid2(frames=[0])
    m.point_cloud = cloud[:, :2]
    agree(m.get_occupancy_grid2(), expect(m, cells, cloud[:, :2]), "n_by_2")


def test_map_without_method_1(ctx, grown):
    """pub_occupancy1=False: the adds take the SLAM cloud and no measurement; the cell lists are the method-1 map's and
    get_occupancy_grid serves method 2"""
    m1, cloud, cells = grown
    m, cloud_again = new_map(ctx, pub_occupancy1=False)
    assert np.array_equal(cloud, cloud_again) and np.array_equal(m.point_cloud, cloud)
    for a, b in zip(m.keyframes, m1.keyframes):
        assert (a is None) == (b is None)
        if a is not None:
            assert np.array_equal(a.r, b.r) and np.array_equal(a.c, b.c)
    for kw in (dict(), dict(frames=[2, 5, 9], resolution=0.45)):
        agree(m.get_occupancy_grid(**kw), expect(m, cells, cloud, **kw), kw)


# ---- three sessions in lock-step --------------------------------------------------------------------------------------------
HISTORIES = [HISTORY,                                                                       # grown
             [(0, "A", (0.0, 0.0, 0.0)), (2, "A", (1.0, 1.0, 0.5)), (3, "B", (2.0, 0.0, -0.5))],   # key 1 missed
             [(0, "B", (0.5, -0.5, 0.2)), (1, "A", (1.5, 0.0, 0.0))]]                       # its cloud is empty
QUERIES = (dict(), dict(frames=[0, 2, 1, 7], resolution=0.5))


def fed_batch(ctx, **over):
    b = MapBatch(ctx, 3, max_keyframes=8, **dict(SETTINGS, **over))
    b.configure()
    clouds = []
    for s, hist in enumerate(HISTORIES):
        local, cloud = history_clouds(hist, 20 + s)
        if s == 2:
            local, cloud = [p[:0] for p in local], cloud[:0]
        clouds.append(cloud)
        for (key, geom, pose), pts in zip(hist, local):
            b.add_keyframes([s], [key], [Pose2(*pose)], PINGS[geom], [cloud if not b.pub_occupancy1 else pts])
    return b, clouds


@pytest.fixture(scope="module")
def singles(ctx):
    """each session's own Mapping, its stored cloud the session's keyed cloud, and the images it publishes"""
    out = []
    for s, hist in enumerate(HISTORIES):
        m, cloud = new_map(ctx, hist, 20 + s)
        if s == 2:
            cloud = cloud[:0]
        m.point_cloud = cloud
        out.append((m, cloud, [m.get_occupancy_grid2(**kw) for kw in QUERIES]))
    return out


def same(a, b):
    assert info_of(a) == info_of(b) and a.occ.shape == b.occ.shape and np.array_equal(a.occ, b.occ) and a.data == b.data


def test_batch_sessions_equal_their_own_maps(ctx, singles):
    b, clouds = fed_batch(ctx)
    assert b.maps[0]._grow != [0, 0] and b.maps[1].keyframes[1] is None and len(clouds[2]) == 0
    for q, kw in enumerate(QUERIES):
        for s in range(3):                          # the stored clouds are the last keyframe's: set the sessions' own
            b.maps[s].point_cloud = clouds[s]
        for s, msg in enumerate(b.get_occupancy_grid2(**kw)):
            same(msg, singles[s][2][q])
        for i, msg in enumerate(b.get_occupancy_grid2(sessions=[2, 0], **kw)):
            same(msg, singles[[2, 0][i]][2][q])
        same(b.maps[1].get_occupancy_grid2(**kw), singles[1][2][q])          # a session's own call goes through the batch
        for s in range(3):
            b.maps[s].point_cloud = None
        for s, msg in enumerate(b.get_occupancy_grid2(point_clouds=clouds, **kw)):
            same(msg, singles[s][2][q])
    with pytest.raises(RuntimeError, match="point_cloud"):
        b.get_occupancy_grid2()
    # session 2 alone is all free cells and unknown
    assert set(np.unique(singles[2][2][0].occ)) == {-1, 0}
    want = mapping2_ref.occupancy_grid2(singles[0][0], cells_of(singles[0][0]), clouds[0], oracle.remove_outlier)
    agree(singles[0][2][0], want)


def test_batch_without_method_1(ctx, singles):
    b, clouds = fed_batch(ctx, pub_occupancy1=False)
    for s in range(3):
        assert np.array_equal(np.asarray(b.maps[s].point_cloud).reshape(-1, 4), clouds[s])
    for q, kw in enumerate(QUERIES):
        for s, msg in enumerate(b.get_occupancy_grids(**kw)):
            same(msg, singles[s][2][q])
        same(b.get_occupancy_grids(sessions=[1], **kw)[0], singles[1][2][q])
