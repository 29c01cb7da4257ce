"""The log-odds map's measure, fit and render kernels (csrc/sfe_map.hip) at the constructed edge cases of
tests/mapping_edges.py, against tests/mapping_ref.py.  tests/test_mapping_edges_host.py shows on the reference alone that every
case holds what it is for."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mapping_edges as E  # noqa: E402
from mapping_edges import data_agrees, same_map, ulps  # noqa: E402
from sonar_slam_amd import _lib  # noqa: E402
from sonar_slam_amd.mapping import MapBatch, Mapping  # noqa: E402
from sonar_slam_amd.pose2 import Pose2  # noqa: E402

pytestmark = pytest.mark.gpu

GROUPS = E.measure_groups()
ORIGIN = Pose2(0.0, 0.0, 0.0)


@pytest.fixture(scope="module")
def ctx():
    return _lib.default_context()


# ---- measurement ------------------------------------------------------------------------------------------------------------
class Singles(object):
    """one Mapping per (image shape, probabilities); a case runs in it through the seam add_keyframe uses:
    _new_keyframe -> _measure(slot, geom, hits, hr, hc) -> measure_stages()"""

    def __init__(self, ctx):
        self.ctx, self.maps = ctx, {}

    def run(self, case):
        key = (case.shape, case.hit_prob, case.miss_prob)
        if key not in self.maps:
            self.maps[key] = E.configured(Mapping(self.ctx), E.measure_settings(case))
        m = self.maps[key]
        kf = E.measure_keyframe(m, case, ORIGIN)
        m._measure(kf._slot, kf.geom, case.hits, case.hr, case.hc)
        return m.measure_stages() + (kf.logodds,)


def against_ref(got, case):
    hits, prob, fh, lo = got
    want_lo, st = E.measure_ref(case)
    assert hits.shape == prob.shape == case.shape and fh.shape == (case.shape[1],)
    if "hits" in st:
        assert np.array_equal(hits, st["hits"].astype(np.uint8)), case.name
        assert np.array_equal(fh, st["first_hits"]), case.name
    else:
        assert not hits.any() and (fh == case.shape[0]).all(), case.name
    assert np.array_equal(prob.view(np.int32), st["prob"].view(np.int32)), case.name
    assert lo.shape == want_lo.shape and ulps(lo, want_lo).max() <= 2, case.name


def same_stages(got, want, tag):
    bits = lambda a: a.view(np.int32) if a.dtype == np.float32 else a
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, tag
        assert np.array_equal(bits(a), bits(b)), tag


@pytest.mark.parametrize("group", list(GROUPS))
def test_measurement_against_mapping_ref(ctx, group):
    """hit mask and first hits equal, the image before logit bit-equal, log-odds within 2 ulp: every layout of one image shape
    and one inflation kernel"""
    singles = Singles(ctx)
    for case in GROUPS[group]:
        against_ref(singles.run(case), case)


@pytest.mark.parametrize("group", list(GROUPS))
def test_measurement_in_a_batch_equals_the_single_map(ctx, group):
    """three sessions in one MapBatch measurement call: the case between a keyframe without points and a many-hits keyframe of
    other geometries, then in the reverse order; each session's stages are bit for bit its single-Mapping run's"""
    singles = Singles(ctx)
    batches = {}
    for case in GROUPS[group]:
        none, many = E.batch_neighbours(case)
        want = {c.name: singles.run(c) for c in (none, case, many)}
        against_ref(want[many.name], many)
        for order, trio in enumerate([(none, case, many), (many, case, none)]):
            key = (order, case.shape, case.hit_prob, case.miss_prob)     # (a slot keeps the geometry it was bound to)
            if key not in batches:
                batches[key] = MapBatch(ctx, 3, 2, max_pixels=2048, **E.measure_settings(case))
                batches[key].configure()
            b = batches[key]
            kfs = [E.measure_keyframe(b.maps[s], c, ORIGIN) for s, c in enumerate(trio)]
            b._hits_many = lambda sessions, clouds, trio=trio: [(c.hits, c.hr, c.hc) for c in trio]
            b._measure_many([0, 1, 2], kfs, [()] * 3)
            for s, c in enumerate(trio):
                b.maps[s]._meas_job = s
                same_stages(b.maps[s].measure_stages() + (kfs[s].logodds,), want[c.name], (case.name, order, s))


# ---- fit, apply, growth -------------------------------------------------------------------------------------------------------
def lockstep(ctx, case):
    """the product and mapping_ref through `case`, compared after every step -> (product map, reference map)"""
    m, ref = E.configured(Mapping(ctx), case.settings), E.ref_map(case.settings)
    for i, st in enumerate(case.steps):
        one = case._replace(steps=[st])
        E.run_session(ref, one, Pose2)
        E.run_session(m, one, Pose2, batched=True)
        same_map(m, ref, (case.name, i, st[0]))
    return m, ref


@pytest.mark.parametrize("case", E.fit_sessions(), ids=lambda c: c.name)
def test_fit_apply_and_growth_against_mapping_ref(ctx, case):
    """after every step: box, size and origin equal, grid bits equal, every keyframe's r / c / l equal; an update step as one
    update_poses call equals the update_pose loop"""
    m, ref = lockstep(ctx, case)
    for kf, rk in zip(m.keyframes, ref.keyframes):
        assert np.array_equal(kf.logodds, rk.logodds)
    if any(st[0] == "update" for st in case.steps):
        loop = E.run_session(E.configured(Mapping(ctx), case.settings), case, Pose2, batched=False)
        same_map(loop, m, (case.name, "update_pose loop"))


def test_fit_sessions_side_by_side_in_a_batch(ctx):
    """the tie, growth and window sessions as three sessions of one MapBatch (different geometries, one growing while the
    others do not): each equals mapping_ref after every round of steps"""
    cases = [E.tie_session(), E.growth_session(), E.window_session()]
    settings = dict(E.TIE_SETTINGS)
    cases = [c._replace(settings=settings) for c in cases]
    b = MapBatch(ctx, len(cases), 12, max_pixels=256, **settings)
    b.configure()
    refs = [E.ref_map(settings) for _ in cases]
    for i in range(max(len(c.steps) for c in cases)):
        live = [(s, c.steps[i]) for s, c in enumerate(cases) if i < len(c.steps)]
        adds = [(s, st) for s, st in live if st[0] == "add"]
        if adds:
            b.add_keyframes_logodds([s for s, _ in adds], [st[1] for _, st in adds], [Pose2(*st[2]) for _, st in adds],
                                    [st[3] for _, st in adds], [st[4] for _, st in adds])
        ups = [(s, k, Pose2(*p)) for s, st in live if st[0] == "update" for k, p in zip(st[1], st[2])]
        if ups:
            b.update_poses([u[0] for u in ups], [u[1] for u in ups], [u[2] for u in ups])
        for s, st in live:
            E.run_session(refs[s], cases[s]._replace(steps=[st]), Pose2)
            same_map(b.maps[s], refs[s], (cases[s].name, i))


# ---- render ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.render_sessions(), ids=lambda c: c.name)
def test_render_against_mapping_ref(ctx, case):
    """info equal, the frames= grid bit-equal, int8 data equal up to near-integer 100 p (data_agrees); nothing excused where
    100 p is exactly 0, 50 or 100"""
    m, ref = lockstep(ctx, case)
    excused = 0
    for kw in case.pubs:
        got, want = m.get_occupancy_grid(**kw), ref.get_occupancy_grid1(**kw)
        assert E.info_of(got) == E.info_of(want), kw
        assert got.occ.dtype == np.int8 and got.occ.shape == (want.info.height, want.info.width), kw
        if kw["frames"] is not None:
            assert np.array_equal(m.frames_grid().view(np.int32), ref.last_frames_grid.view(np.int32)), kw
        p100 = (100 * want.probs).astype(np.float32)
        excused += data_agrees(got.data, want.data, p100.ravel())
    if case.name == "render_saturated":
        assert excused == 0
    same_map(m, ref, (case.name, "after publishing"))


def test_render_in_a_batch_equals_the_single_map(ctx):
    """the render sessions that share the 0.5 m settings as sessions of one MapBatch: get_occupancy_grids equals each single
    Mapping's image, byte for byte (crops of different sizes, an empty one among them, in one launch)"""
    cases = [E.render_session(), E.pixel_session(), E.saturation_session()]
    settings = cases[0].settings
    b = MapBatch(ctx, len(cases), 6, max_pixels=512, **settings)
    b.configure()
    singles = []
    for s, c in enumerate(cases):
        c = c._replace(settings=settings)
        E.run_session(b.maps[s], c, Pose2)
        singles.append(E.run_session(E.configured(Mapping(ctx), settings), c, Pose2))
        same_map(b.maps[s], singles[s], c.name)
    for kw in cases[0].pubs[:25] + cases[1].pubs:
        got = b.get_occupancy_grids(**kw)
        for s, m in enumerate(singles):
            want = m.get_occupancy_grid(**kw)
            assert E.info_of(got[s]) == E.info_of(want) and np.array_equal(got[s].occ, want.occ), (kw, s)


# ---- what reference and product refuse alike --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ping,error", E.REFUSED_PINGS, ids=[r[0] for r in E.REFUSED_PINGS])
def test_pings_below_four_beams_are_refused_like_the_reference(ctx, name, ping, error):
    m = E.configured(Mapping(ctx), E.TIE_SETTINGS)
    with pytest.raises(error):
        m.add_keyframe_logodds(0, Pose2(0.0, 0.0, 0.0), ping, np.ones(8, np.float32))
    assert m.keyframes == [] and not m.logodds_grid.any()


def test_finer_resolutions_are_refused_like_the_reference(ctx):
    case = E.pixel_session()
    m, ref = lockstep(ctx, case)
    for r in E.REFUSED_RESOLUTIONS:
        for obj, call in ((m, m.get_occupancy_grid), (ref, ref.get_occupancy_grid1)):
            with pytest.raises(AssertionError):
                call(resolution=r)
    same_map(m, ref)
