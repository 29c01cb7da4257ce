"""Method 2 from a cloud in a CloudStore (Mapping / MapBatch.get_occupancy_grid2_store: sfe_map_render2_store /
sfe_mapset_render2_store in csrc/sfe_map.hip; CloudStore.put_keys): bit for bit the reference's recorded publications
(tests/golden/mapping2_session.npz) and the host-fed get_occupancy_grid2 on the cloud read back."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mapping_ref  # noqa: E402
import test_gpu_mapping2 as base  # noqa: E402
from sonar_slam_amd import _lib  # noqa: E402
from sonar_slam_amd.mapping import Mapping  # noqa: E402
from sonar_slam_amd.pose2 import Pose2  # noqa: E402
from sonar_slam_amd.store import CloudStore, pose_T6  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return _lib.default_context()


@pytest.fixture(scope="module")
def store(ctx):
    s = CloudStore(ctx, capacity_points=1 << 15, max_clouds=64)
    yield s
    s.close()


def read_back(store, handle, keyed=True):
    """the cloud the host-fed call is given: x, y, 0, key as float32 (without keys: x, y)"""
    pts = store.read(handle)
    return np.c_[pts, np.zeros(len(pts)), store.read_keys(handle)].astype(np.float32) if keyed else pts


def same(a, b, tag=None):
    assert base.info_of(a) == base.info_of(b), tag
    assert a.occ.dtype == np.int8 and a.occ.shape == b.occ.shape, tag
    assert np.array_equal(a.occ, b.occ), (tag, np.argwhere(a.occ != b.occ)[:8])
    assert a.data == b.data and a.header.frame_id == b.header.frame_id == "map", tag


# ---- the reference's session ------------------------------------------------------------------------------------------------
def test_session_publications_equal_the_reference(ctx, store):
    """every publication of both stages whose cloud is float32 (`cloud32`) or empty, through put_keys and the store route:
    data bit for bit, info and the known region's box.  `frames` has a repeat, a missed key and a key beyond the session;
    `coarse` / `frames_coarse` / `near` the resize and its threshold; the 2263-point cloud crosses the radius count's
    2048-point tile.  The two `cloud64` publications are float64 clouds, which a float32 store cannot hold: they are the
    only ones left out."""
    first = np.load(os.path.join(HERE, "golden", "mapping_session.npz"))
    fix = np.load(os.path.join(HERE, "golden", "mapping2_session.npz"))
    pubs = json.loads(str(fix["pubs"]))
    assert sorted(n for n, p in pubs.items() if p[1] == "cloud64") == ["frames_nofilter64", "nofilter64"]
    steps = json.loads(str(first["steps"]))
    ends = {max(i for i, s in enumerate(steps) if s["op"] == "add"): "adds",
            max(i for i, s in enumerate(steps) if s.get("pass_") == "lc"): "lc"}
    m = Mapping(ctx)
    for k, v in json.loads(str(fix["settings"])).items():
        setattr(m, k, v)
    m.configure()
    keep = dict(outlier_filter_min_points=m.outlier_filter_min_points, dilate_size=m.dilate_size)
    done, n_slots = [], len(store)

    def check(i, st):
        stage = ends.get(i)
        if stage is None:
            return
        cloud = fix["cloud32_%s" % stage]
        assert cloud.dtype == np.float32 and len(cloud) > 2048
        handles = {"cloud32": store.put_keys(cloud[:, :2], np.uint32(cloud[:, 3])),
                   "empty": store.put_keys(np.zeros((0, 2), np.float32), np.zeros(0, np.uint32))}
        assert np.array_equal(read_back(store, handles["cloud32"]), cloud)
        for name, (kw, which, over) in pubs.items():
            if which == "cloud64":
                continue
            for k, v in dict(keep, **over).items():
                setattr(m, k, v)
            tag = "pub_%s_%s_" % (stage, name)
            msg = m.get_occupancy_grid2_store(store, handles[which], **kw)
            assert list(m._render2_plan(kw.get("frames"), kw.get("resolution"))[1]) == list(fix[tag + "box"]), tag
            assert base.info_of(msg) == list(fix[tag + "info"]), tag
            got, want = msg.occ.ravel(), fix[tag + "data"]
            assert got.dtype == np.int8 and got.shape == want.shape and np.array_equal(got, want), (tag, int((got != want).sum()))
            assert msg.data == list(want) and msg.header.frame_id == "map" and msg.info.origin.orientation.w == 1
            done.append((stage, name))
        for k, v in keep.items():
            setattr(m, k, v)
        store.truncate(n_slots)

    mapping_ref.replay(m, first, Pose2, check=check)
    names = [n for n, p in pubs.items() if p[1] != "cloud64"]
    assert done == [(st, n) for st in ("adds", "lc") for n in names] and len(names) == len(pubs) - 2
    assert m.point_cloud is not None        # (what add_keyframe stored: the store route neither reads nor sets it)
    m.close()


# ---- against the host-fed call on a grown map -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grown(ctx, store):
    """test_gpu_mapping2.py's grown map (key 3 missed; origin moved on top and on the left) and, in the store, its keyed
    cloud with two additions: points keyed 3 (a key with points but no keyframe) and, keyed 4, points one cell outside the
    known region (and one inside)"""
    m, cloud = base.new_map(ctx)
    assert m._grow[0] > 0 and m._grow[1] > 0 and m.keyframes[0].base == (0, 0) and m.keyframes[3] is None
    rng = np.random.default_rng(8)
    extra3 = base.registered(base.fan_points(rng, 40, 8.0), base.HISTORY[1][2], 3)
    out = base.outside_points(m)
    extra4 = np.c_[out, np.zeros(len(out)), np.full(len(out), 4.0)].astype(np.float32)
    y0, x0, h, w = base.region(m)
    r, c = np.rint((extra4[:, 1] - y0) / m.resolution), np.rint((extra4[:, 0] - x0) / m.resolution)
    assert ((r >= 0) & (r < h) & (c >= 0) & (c < w)).sum() == 1 and len(extra4) == 7
    full = np.concatenate([cloud, extra3, extra4])
    handle = store.put_keys(full[:, :2], full[:, 3])
    assert np.array_equal(read_back(store, handle), full)
    return m, handle, full, base.cells_of(m)


GROWN_CASES = {
    # name: (settings changed, arguments)
    "all_frames": (dict(), dict()),
    "frames_1_0": (dict(), dict(frames=[1, 0])),
    "frames_0_0_2": (dict(), dict(frames=[0, 0, 2])),
    "frames_3_1": (dict(), dict(frames=[3, 1])),
    "frames_negative": (dict(), dict(frames=[-1, 2])),
    "filter_off": (dict(outlier_filter_min_points=1), dict()),
    "filter_off_frames": (dict(outlier_filter_min_points=1), dict(frames=[4, 4, 0])),
    "filter_empties_the_cloud": (dict(outlier_filter_min_points=100000), dict()),
    "dilate_1": (dict(dilate_size=1), dict()),
    "dilate_7": (dict(dilate_size=7), dict(frames=[5, 2, 4])),
    "outside_points": (dict(outlier_filter_min_points=1, dilate_size=1), dict()),
    "resized": (dict(), dict(resolution=0.5)),
    "resized_frames": (dict(), dict(frames=[2, 5, 2], resolution=0.5)),
}


def both_routes(m, store, handle, over, kw, keyed=True):
    keep = {k: getattr(m, k) for k in over}
    try:
        for k, v in over.items():
            setattr(m, k, v)
        m.point_cloud = read_back(store, handle, keyed)
        want = m.get_occupancy_grid2(**kw)
        marker = m.point_cloud = np.zeros((1, 4), np.float32)
        got = m.get_occupancy_grid2_store(store, handle, **kw)
        assert m.point_cloud is marker          # the store route does not touch it
    finally:
        for k, v in keep.items():
            setattr(m, k, v)
    return got, want


@pytest.mark.parametrize("name", sorted(GROWN_CASES))
def test_grown_map_equals_the_host_fed_call(grown, store, name):
    m, handle, full, cells = grown
    over, kw = GROWN_CASES[name]
    got, want = both_routes(m, store, handle, over, kw)
    same(got, want, name)
    values = set(np.unique(want.occ))
    if name == "filter_empties_the_cloud":
        assert values == {-1, 0}
    else:
        assert values == {-1, 0, 100}, name
    if name == "frames_0_0_2":
        # the doubled key changes the filter's decision, so the image shows the multiplicity: with the restatement first
        twice, once = base.expect(m, cells, full, **kw), base.expect(m, cells, full, frames=[0, 2])
        assert twice["data"].shape == once["data"].shape
        assert not np.array_equal(twice["data"], once["data"])
        base.agree(want, twice, name)
        assert not np.array_equal(got.occ, m.get_occupancy_grid2_store(store, handle, frames=[0, 2]).occ)
    if name == "frames_3_1":
        # the points keyed 3 are projected although no keyframe 3 exists
        assert (got.occ == 100).sum() > (m.get_occupancy_grid2_store(store, handle, frames=[1]).occ == 100).sum()


def test_frames_that_select_no_point_give_free_cells_only(grown, store):
    """key 3 alone marks nothing (IndexError on both routes); a listed keyframe whose key no point carries gives its free
    cells and nothing else"""
    m, handle, full, _ = grown
    for route in (lambda: m.get_occupancy_grid2_store(store, handle, frames=[3]), lambda: m.get_occupancy_grid2(frames=[3])):
        m.point_cloud = full
        with pytest.raises(IndexError):
            route()
    n = len(store)
    part = full[full[:, 3] != 1]
    h = store.put_keys(part[:, :2], part[:, 3])
    got, want = both_routes(m, store, h, dict(), dict(frames=[1]))
    same(got, want)
    assert set(np.unique(got.occ)) == {-1, 0}
    got, want = both_routes(m, store, h, dict(), dict(frames=[1, 1, 77, -4]))
    same(got, want)
    assert set(np.unique(got.occ)) == {-1, 0}
    store.truncate(n)


def test_cloud_made_by_get_points_keys(ctx, grown, store):
    """the keyframe clouds put into the store, registered and downsampled there at point_resolution 0.5"""
    m = grown[0]
    n = len(store)
    local, _ = base.history_clouds(base.HISTORY, 3)
    handles = [store.put(p) for p in local]
    keys = [key for key, _, _ in base.HISTORY]
    h = store.get_points_keys(handles, [pose_T6(Pose2(*pose)) for _, _, pose in base.HISTORY], keys, 0.5)
    cloud = read_back(store, h)
    assert 50 < len(cloud) < 300 and sorted(set(cloud[:, 3])) == keys
    for kw in (dict(), dict(frames=[4, 0, 4, 3]), dict(frames=[1, 2], resolution=0.5)):
        got, want = both_routes(m, store, h, dict(), kw)
        same(got, want, kw)
        assert (got.occ == 100).any()
    # an unkeyed cloud serves all frames
    got, want = both_routes(m, store, handles[0], dict(outlier_filter_min_points=3), dict(), keyed=False)
    same(got, want)
    assert (got.occ == 100).any()
    store.truncate(n)


# ---- three sessions in one call ---------------------------------------------------------------------------------------------
def test_batch_equals_one_map_calls_and_the_host_fed_batch(ctx, store):
    b, clouds = base.fed_batch(ctx)
    assert len(clouds[2]) == 0          # session 2: an empty selection whatever the frames
    n = len(store)
    handles = [store.put_keys(c[:, :2], c[:, 3]) for c in clouds]
    singles = []
    for s, hist in enumerate(base.HISTORIES):
        singles.append(base.new_map(ctx, hist, 20 + s)[0])
    for kw in base.QUERIES + (dict(frames=[2, 2, 0]),):
        got = b.get_occupancy_grid2_store(store, handles, **kw)
        host = b.get_occupancy_grid2(point_clouds=clouds, **kw)
        assert len(got) == 3
        for s in range(3):
            same(got[s], host[s], (s, kw))
            same(got[s], singles[s].get_occupancy_grid2_store(store, handles[s], **kw), (s, kw))
            same(got[s], b.maps[s].get_occupancy_grid2_store(store, handles[s], **kw), (s, kw))      # through the batch
        assert (got[0].occ == 100).any() and (got[1].occ == 100).any() and set(np.unique(got[2].occ)) == {-1, 0}
        part = b.get_occupancy_grid2_store(store, [handles[2], handles[0]], sessions=[2, 0], **kw)
        same(part[0], host[2])
        same(part[1], host[0])
    with pytest.raises(ValueError, match="sessions but a list"):
        b.get_occupancy_grid2_store(store, handles[:2])
    store.truncate(n)
    for m in singles:
        m.close()
    b.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(ctx, grown, store):
    m, handle, full, _ = grown
    plain = store.put(full[:, :2])
    n = len(store)
    grid = m.logodds_grid.copy()
    shape = tuple(m.logodds_grid.shape)
    want = m.get_occupancy_grid2_store(store, handle, frames=[0, 1])

    def unchanged():
        assert len(store) == n and tuple(m.logodds_grid.shape) == shape and np.array_equal(m.logodds_grid, grid)
        same(m.get_occupancy_grid2_store(store, handle, frames=[0, 1]), want)

    with pytest.raises(_lib.SonarFEError, match="cloud %d named" % (n + 3)):
        m.get_occupancy_grid2_store(store, n + 3)
    unchanged()
    with pytest.raises(_lib.SonarFEError, match="cloud -1 named"):
        m.get_occupancy_grid2_store(store, -1, frames=[0])
    unchanged()
    with pytest.raises(_lib.SonarFEError, match="has no keys"):
        m.get_occupancy_grid2_store(store, plain, frames=[0, 1])
    unchanged()
    other_ctx = _lib.Context(ctx.device)
    other = CloudStore(other_ctx, capacity_points=1 << 12, max_clouds=4)
    h_other = other.put_keys(full[:, :2], full[:, 3])
    with pytest.raises(ValueError, match="another context"):
        m.get_occupancy_grid2_store(other, h_other)
    assert len(other) == 1
    unchanged()
    with pytest.raises(IndexError, match="known region"):
        m.get_occupancy_grid2_store(store, handle, frames=[3, 99])
    unchanged()
    with pytest.raises(ValueError, match="keys must be integers"):
        store.put_keys(full[:2, :2], [-1, 2])
    with pytest.raises(ValueError, match="points but"):
        store.put_keys(full[:2, :2], [1])
    unchanged()
    other.close()
    store.truncate(n - 1)
