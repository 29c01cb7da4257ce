"""Constructed edge cases of the log-odds map (method 1): small records that tests/test_mapping_edges_host.py runs through
tests/mapping_ref.py alone (to show that each case holds what it is for) and tests/test_gpu_mapping_edges.py runs through the
device (csrc/sfe_map.hip: map_hits / map_filter / map_columns, map_cell / map_scatter / map_compact, mapset_render) against
mapping_ref.  Importable without a GPU.  Also home of ``ulps`` and ``data_agrees``, shared with tests/test_gpu_mapping.py.

What could not be constructed, and what stands in for it:
  * a ping of one beam (a fit window one column wide at yaw 0, a 9 x 1 image): ``interp1d(kind="cubic")`` needs four bearings,
    so the reference raises ValueError in ``oculus.configure`` and so does the product (REFUSED_PINGS).  No skip gives one beam
    column with more than one range row either: c_skip >= n_beams needs max_range <= 0.44 resolution, and then r_skip >=
    n_ranges.  The 9 x 1 measurement image is therefore registered as a geometry directly (Measure.ping is None), and the
    one-column / one-row fit windows come from a narrow fan on a coarse map (fit case "window_one_wide").
  * a render whose source index is clamped to n - 1: with ratio f <= 1 the last output index is at most n f - 0.5, so
    floor(i / f) <= n - 0.5 / f < n.  The clamp never binds for a resolution the reference accepts (clamp_never_binds below
    is checked by the host test); a finer resolution than the map's is refused by an assert in reference and product alike
    (REFUSED_RESOLUTIONS).
  * a pre-clip value of exactly 0.5 at the default hit_prob = 0.8: it needs a subset of OpenCV's fixed taps that sums to 5/8
    of the centre tap, and there is none (the host test searches the fixed kernels).  With hit_prob = 0.75 the 1 x 5 kernel
    gives it exactly: 0.25 / (0.375 / 0.75) = 0.5 in every arithmetic (measure case "exactly_half").
"""
import collections
import os
import re

import numpy as np

import mapping_ref
from mapping_ref import SessionPing

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- comparison rules shared with tests/test_gpu_mapping.py ----------------------------------------------------------------
def ulps(a, b):
    ia = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def data_agrees(got, want, p100):
    """int8 data equal, except where the reference's float32 100 p lies within a few ulp of an integer: there each cell may
    differ by one.  -> number of such cells that differ"""
    got, want = np.asarray(got, np.int64), np.asarray(want, np.int64)
    assert got.shape == want.shape
    diff = got != want
    near = ulps(p100, np.round(p100).astype(np.float32)) <= 4
    assert not (diff & ~near).any(), np.nonzero(diff & ~near)
    assert (np.abs(got - want)[diff] == 1).all()
    return int(diff.sum())


def compact_threads():
    """COMPACT_THREADS of csrc/sfe_map.hip: the workgroup size of map_compact_kernel's scan"""
    src = os.path.join(HERE, os.pardir, "sonar_slam_amd", "csrc", "sfe_map.hip")
    with open(src) as fh:
        return int(re.search(r"constexpr\s+int\s+COMPACT_THREADS\s*=\s*(\d+)\s*;", fh.read()).group(1))


def configured(m, settings):
    for k, v in settings.items():
        setattr(m, k, v)
    m.configure()
    return m


def ref_map(settings):
    return configured(mapping_ref.Mapping(), settings)


def image_shape(settings, ping):
    """the downsampled polar image's shape of `ping` on a map with `settings`"""
    m = ref_map(settings)
    m.geometry(ping, mapping_ref.Submap())
    return tuple(int(v) for v in m.oculus_image_size)


def same_map(m, ref, tag=None):
    """a product map against mapping_ref's (or another product map): box, size, origin, grid bits, every keyframe's r / c / l"""
    assert [int(m.rmin), int(m.rmax), int(m.cmin), int(m.cmax), m.rows, m.cols, m.x0, m.y0] == \
        [int(ref.rmin), int(ref.rmax), int(ref.cmin), int(ref.cmax), ref.rows, ref.cols, ref.x0, ref.y0], tag
    a, b = m.logodds_grid, ref.logodds_grid
    assert a.shape == b.shape and a.dtype == b.dtype == np.float32, tag
    assert np.array_equal(a.view(np.int32), b.view(np.int32)), tag
    assert len(m.keyframes) == len(ref.keyframes), tag
    for k, (kf, rk) in enumerate(zip(m.keyframes, ref.keyframes)):
        assert (kf is None) == (rk is None), (tag, k)
        if kf is not None:
            for name in "rcl":
                got, want = getattr(kf, name), getattr(rk, name)
                assert got.dtype == want.dtype and np.array_equal(got, want), (tag, k, name)


# ---- measurement cases ---------------------------------------------------------------------------------------------------
MEASURE_SETTINGS = dict(x0=-10.0, y0=-10.0, width=20.0, height=20.0, inc=5.0, resolution=0.2)
# image shape -> the ping that gives it on a 0.2 m map (both skips 1); None: no ping can (module docstring)
SHAPES = collections.OrderedDict([((7, 5), SessionPing(5, 7, 0.25)), ((24, 17), SessionPing(17, 24, 0.25)),
                                  ((40, 33), SessionPing(33, 40, 0.25)), ((1, 9), SessionPing(9, 1, 1.0)), ((9, 1), None)])
# (hr, hc); None: hr = rows and hc = cols, a window larger than the image on both axes.  Sizes 1, 3, 5, 7 take OpenCV's fixed
# taps, 9 and above (hr or hc >= 4) the computed ones
PAIRS = [(0, 0), (0, 2), (3, 0), (1, 1), (2, 3), (4, 4), (5, 2), None]

Measure = collections.namedtuple("Measure", "name shape ping layout hits hr hc hit_prob miss_prob")


def layouts(rows, cols):
    """name -> hit cells [n x 2] (row, column) of a rows x cols image; None: a keyframe without points"""
    rng = np.random.default_rng(rows * 100 + cols)
    rr, cc = np.mgrid[:rows, :cols]
    every = np.c_[rr.ravel(), cc.ravel()]
    one = lambda r, c: np.array([[r, c]])
    dup = np.c_[rng.integers(0, rows, 3 * rows * cols), rng.integers(0, cols, 3 * rows * cols)][: max(8, rows * cols)]
    dup = np.concatenate([dup, dup[::2], dup[:3]])
    # one cell in ten, none in the top rows: windows hold a few far hits whose sum stays between 0.5 and hit_prob, below first
    # hits that are not in row 0, so the float32 order of the sum reaches the image before logit
    scatter = every[(every[:, 0] >= min(6, rows - 1)) & (rng.random(len(every)) < 0.1)]
    scatter = scatter if len(scatter) else every[-1:]
    return collections.OrderedDict([
        ("corner_tl", one(0, 0)), ("corner_tr", one(0, cols - 1)), ("corner_bl", one(rows - 1, 0)),
        ("corner_br", one(rows - 1, cols - 1)), ("edge_top", one(0, cols // 2)), ("edge_bottom", one(rows - 1, cols // 2)),
        ("edge_left", one(rows // 2, 0)), ("edge_right", one(rows // 2, cols - 1)),
        ("row0", every[every[:, 0] == 0]), ("last_row", every[every[:, 0] == rows - 1]),
        ("full_column", every[every[:, 1] == cols // 2]), ("checkerboard", every[(every[:, 0] + every[:, 1]) % 2 == 0]),
        ("every", every), ("duplicates", dup), ("scatter", scatter), ("empty", np.zeros((0, 2), np.int64)),
        ("no_points", None)])


def _measure(name, shape, layout, hits, hr, hc, hit_prob=0.8, miss_prob=0.3):
    hits = None if hits is None else np.ascontiguousarray(hits, np.int32).reshape(-1, 2)
    return Measure(name, shape, SHAPES[shape], layout, hits, hr if hits is not None else -1, hc if hits is not None else 0,
                   hit_prob, miss_prob)


def measure_groups():
    """(group name) -> the cases of one image shape and one (hr, hc): every layout"""
    groups = collections.OrderedDict()
    for shape in SHAPES:
        for pair in PAIRS:
            hr, hc = shape if pair is None else pair
            tag = "%dx%d-hr%d-hc%d" % (shape + (hr, hc))
            groups[tag] = [_measure("%s-%s" % (tag, lay), shape, lay, hits, hr, hc)
                           for lay, hits in layouts(*shape).items()]
    # a column whose only value above 0.5 comes from its neighbour's inflation: 4/6 of the centre tap, 0.533 at hit_prob 0.8
    # (columns 1 and 3; columns 0 and 4 get 1/6, 0.133 before the clip and exactly 0.5 after it)
    # ... and the same hit at hit_prob 0.75, where columns 1 and 3 are exactly 0.5 before the clip: not above it, so no hit
    groups["specials"] = [_measure("neighbour_lit", (7, 5), "neighbour_lit", [[3, 2]], 0, 2),
                          _measure("neighbour_lit_2d", (24, 17), "neighbour_lit", [[9, 8], [20, 3]], 3, 2),
                          _measure("exactly_half", (7, 5), "exactly_half", [[3, 2]], 0, 2, hit_prob=0.75),
                          _measure("exactly_half_rows", (24, 17), "exactly_half", [[9, 8], [23, 0]], 2, 0, hit_prob=0.75)]
    return groups


def measure_ref(case):
    """mapping_ref.measurement of a case -> (log-odds, stages)"""
    stages = {}
    rc = None if case.hits is None else (case.hits[:, 0], case.hits[:, 1])
    lo = mapping_ref.measurement(case.shape, rc, case.hr, case.hc, case.hit_prob, case.miss_prob, stages)
    return lo, stages


def measure_settings(case):
    return dict(MEASURE_SETTINGS, hit_prob=case.hit_prob, miss_prob=case.miss_prob)


def fixed_xy(shape):
    """a sonar_xy table for an image shape no ping gives (the measurement never reads it)"""
    rr, cc = np.mgrid[:shape[0], :shape[1]]
    return np.ascontiguousarray(np.c_[0.25 * (1 + rr.ravel()), 0.25 * cc.ravel()].astype(np.float32))


def measure_keyframe(m, case, pose):
    """the keyframe a measurement case runs in on product map `m` (a Mapping or a MapBatch session): _new_keyframe with the
    case's ping; for a shape no ping gives, the geometry is registered the way _new_keyframe registers one"""
    ping = case.ping if case.ping is not None else SHAPES[(7, 5)]
    kf = m._new_keyframe(pose, ping)
    if case.ping is None:
        xy = fixed_xy(case.shape)
        if getattr(m, "_edge_geom", None) is None:
            m._edge_geom = m._register_geometry(xy, case.shape)
        m._geom = m._edge_geom
        m._geom_shape[m._geom] = case.shape
        m.oculus_image_size = case.shape
        kf.geom = m._geom
    assert tuple(m.oculus_image_size) == case.shape
    return kf


# the neighbours of a case in a MapBatch measurement call: a keyframe without points and a many-hits one of other geometries
def batch_neighbours(case):
    many = layouts(12, 11)
    hits = np.concatenate([many["every"], many["duplicates"]])
    a = Measure("none", (5, 9), SessionPing(9, 5, 0.25), "no_points", None, -1, 0, case.hit_prob, case.miss_prob)
    b = Measure("many", (12, 11), SessionPing(11, 12, 0.25), "every", np.ascontiguousarray(hits, np.int32), 2, 1,
                case.hit_prob, case.miss_prob)
    return a, b


# ---- sessions: fit, apply, growth, render -------------------------------------------------------------------------------------
Session = collections.namedtuple("Session", "name settings steps pubs")
PI = float(np.pi)


class _Builder(object):
    def __init__(self, name, **settings):
        self.name, self.settings, self.steps, self.pubs = name, settings, [], []

    def add(self, key, pose, ping, logodds=None):
        """a keyframe from a log-odds image; by default pixel p holds p + 1, so kf.l names the pixel that won its cell"""
        n = int(np.prod(image_shape(self.settings, ping)))
        lo = np.arange(n, dtype=np.float32) + 1 if logodds is None else np.resize(np.asarray(logodds, np.float32), n)
        self.steps.append(("add", key, tuple(float(v) for v in pose), ping, lo))
        return self

    def update(self, keys, poses):
        self.steps.append(("update", list(keys), [tuple(float(v) for v in p) for p in poses]))
        return self

    def pub(self, **kw):
        self.pubs.append(kw)
        return self

    def done(self):
        return Session(self.name, self.settings, self.steps, self.pubs)


def run_session(m, case, pose2, batched=True, check=None):
    """drive `m` (configured from case.settings) through the case; check(step index) after every step.  An update step is one
    update_poses call where `m` has it and `batched` says so, the loop of update_pose calls otherwise."""
    for i, st in enumerate(case.steps):
        if st[0] == "add":
            _, key, pose, ping, lo = st
            m.add_keyframe_logodds(key, pose2(*pose), ping, lo)
        elif batched and hasattr(m, "update_poses"):
            m.update_poses(st[1], [pose2(*p) for p in st[2]])
        else:
            for k, p in zip(st[1], st[2]):
                m.update_pose(k, pose2(*p))
        if check is not None:
            check(i)
    return m


def quotients(m, sonar_xy, pose):
    """the fit's quotients before rounding, as mapping_ref.fit_grid takes them in float64 -> (qr, qc) per pixel"""
    yaw = pose.theta()
    c, s = np.cos(yaw), np.sin(yaw)
    xy = np.array([[c, -s], [s, c]]).dot(sonar_xy.T).T + np.array([pose.x(), pose.y()])
    return (xy[:, 1] - m.y0) / m.resolution, (xy[:, 0] - m.x0) / m.resolution


# ties: 0.5 m ranges under a 0.5 m map.  On the bearing-0 beam X = 0.5 (1 + i) and Y = 0 exactly; at yaw 0 a translation of
# an odd multiple of 0.25 puts those pixels on k + 0.5, k of both parities.  At yaw pi (cos = -1 exactly) the beam runs down
# the columns and its last pixel sits on -0.5 in c; at yaw -pi/2 (sin = -1 exactly) the same in r.  -0.5 rounds to -0 = 0:
# no growth.
TIE_PING = SessionPing(5, 8, 0.5)
TIE_SETTINGS = dict(x0=-4.0, y0=-4.0, width=12.0, height=12.0, inc=4.0, resolution=0.5)


def tie_session():
    b = _Builder("ties", **TIE_SETTINGS)
    b.add(0, (0.25, 0.25, 0.0), TIE_PING)       # c: 9.5 + i, r: 8.5
    b.add(1, (0.5, 0.75, 0.0), TIE_PING)        # c: whole numbers, r: 9.5
    b.add(2, (-0.25, 0.0, PI), TIE_PING)        # c: 6.5 - i: down to -0.5
    b.add(3, (0.0, -0.25, -PI / 2), TIE_PING)   # r: 6.5 - i: down to -0.5
    b.update([1, 0], [(0.75, 0.25, 0.0), (1.25, 1.75, 0.0)])
    return b.done()


def tie_session_quarter():
    """the same on a 0.25 m map under 0.25 m ranges"""
    ping = SessionPing(7, 12, 0.25)
    b = _Builder("ties_quarter", x0=-4.0, y0=-4.0, width=8.0, height=8.0, inc=4.0, resolution=0.25)
    b.add(0, (0.125, 0.375, 0.0), ping)
    b.add(1, (-0.875, 0.0, PI), ping)           # last pixel of the beam: (-3 - 0.875 + 4) / 0.25 = 0.5; none at -0.5
    b.add(2, (-1.125, 0.0, PI), ping)           # ... (-3 - 1.125 + 4) / 0.25 = -0.5
    b.add(3, (0.0, -1.125, -PI / 2), ping)
    return b.done()


def dedup_session():
    """a 1.0 m map under 0.25 m ranges and 33 beams: dozens of pixels per cell near the sonar, the smallest index wins"""
    ping = SessionPing(33, 40, 0.25)
    b = _Builder("coarse", x0=-10.0, y0=-10.0, width=20.0, height=20.0, inc=5.0, resolution=1.0)
    b.add(0, (0.1, 0.2, 0.3), ping).add(1, (-3.0, 2.0, -2.0), ping)
    b.update([0], [(1.0, -1.0, 1.0)])
    return b.done()


def fine_session():
    """a 0.2 m map under 0.5 m ranges and 5 beams: (almost) every pixel has its own cell"""
    ping = SessionPing(5, 16, 0.5)
    b = _Builder("fine", x0=-10.0, y0=-10.0, width=20.0, height=20.0, inc=4.0, resolution=0.2)
    b.add(0, (0.03, 0.07, 0.3), ping).add(1, (-1.0, 0.5, 2.0), ping)
    b.update([1], [(0.0, 0.0, -1.0)])
    return b.done()


def window_session():
    """a narrow fan on a coarse map: every pixel in one column (yaw 0) or in one row (yaw pi/2); then all in one cell"""
    ping = SessionPing(5, 2, 0.6)       # X in [0.25, 1.2], Y in [-1.09, 1.09]
    b = _Builder("window_one_wide", x0=-5.0, y0=-5.0, width=10.0, height=10.0, inc=4.0, resolution=1.0)
    b.add(0, (-0.72, 0.0, 0.0), ping)
    b.add(1, (0.0, -0.72, PI / 2), ping)
    b.add(2, (0.3, 0.3, 0.7), SessionPing(5, 3, 0.05))
    b.update([0], [(2.28, 1.0, 0.0)])
    return b.done()


# occupied-cell count of the one keyframe -> (range_resolution, n_beams, n_ranges trimmed to hit it, pose), on a 0.2 m map:
# 63 / 64 / 65 around a wave of map_compact_kernel's scan, 1023 / 1024 / 1025 around its workgroup (found by a search over
# n_ranges and small pose offsets with mapping_ref; the host test holds each count to its name)
COMPACT_GEOMETRIES = collections.OrderedDict([
    (63, (0.2, 7, 10, (0.03, 0.07, 0.3))), (64, (0.2, 7, 10, (0.0, 0.0, 0.0))), (65, (0.2, 13, 7, (0.0, 0.0, 0.0))),
    (1023, (0.2, 33, 39, (-9.39, 0.143, 0.22))), (1024, (0.2, 33, 39, (-9.4, 0.13, 0.2))),
    (1025, (0.25, 33, 36, (-9.4, 0.13, 0.2)))])


def compact_sessions():
    out = []
    for count, (rr, nb, nr, pose) in COMPACT_GEOMETRIES.items():
        b = _Builder("compact_%d" % count, x0=-10.0, y0=-10.0, width=20.0, height=20.0, inc=5.0, resolution=0.2)
        out.append((count, b.add(0, pose, SessionPing(nb, nr, rr)).done()))
    return out


# growth: a 20 x 20 grid at 0.5 m, inc = 4 m = 8 cells; the beam's last pixel is 2 m out.  One step: a cell at exactly -1 or at
# exactly rows / cols.  Two steps in one fit: a keyframe more than inc outside.  Then one update_poses call that moves a
# keyframe out (two steps on the left) and another back to the middle.
GROW_PING = SessionPing(5, 4, 0.5)
GROW_SETTINGS = dict(x0=-5.0, y0=-5.0, width=10.0, height=10.0, inc=4.0, resolution=0.5)
# (key, pose, rows grown on top, at the bottom, columns grown on the left, on the right)
GROW_STEPS = [(0, (0.0, 0.0, 0.0), 0, 0, 0, 0),
              (1, (0.0, -3.5, -PI / 2), 8, 0, 0, 0),      # y0 = -5: (-2 - 3.5 + 5) / 0.5 = -1
              (2, (0.0, 3.0, PI / 2), 0, 8, 0, 0),        # y0 = -9, 28 rows: (2 + 3 + 9) / 0.5 = 28
              (3, (-3.5, 0.0, PI), 0, 0, 8, 0),
              (4, (3.0, 0.0, 0.0), 0, 0, 0, 8),
              (5, (0.0, -14.0, -PI / 2), 16, 0, 0, 0),    # y0 = -9: (-2 - 14 + 9) / 0.5 = -14
              (6, (0.0, 11.5, PI / 2), 0, 16, 0, 0),      # y0 = -17, 52 rows: (2 + 11.5 + 17) / 0.5 = 61 >= 52 + 8
              (7, (-14.0, 0.0, PI), 0, 0, 16, 0),
              (8, (11.5, 0.0, 0.0), 0, 0, 0, 16)]


def growth_session():
    b = _Builder("growth", **GROW_SETTINGS)
    for key, pose, _, _, _, _ in GROW_STEPS:
        b.add(key, pose, GROW_PING)
    b.update([0, 5, 0], [(-24.0, 0.0, PI), (0.5, 0.5, 0.1), (0.0, 30.0, PI / 2)])
    return b.done()


def fit_sessions():
    return ([tie_session(), tie_session_quarter(), dedup_session(), fine_session(), window_session(), growth_session()]
            + [s for _, s in compact_sessions()])


# ---- render ---------------------------------------------------------------------------------------------------------------
# one pixel per keyframe: c_skip = 8 >= 5 beams, r_skip = 4 >= 1 range; the pixel lies 0.125 m from the pose at -65 degrees
PIXEL_PING = SessionPing(5, 1, 0.125)
RENDER_FACTORS = (1.0, 1.09, 1.11, 2.0, 1.5)


def _varied(n, seed):
    return np.random.default_rng(seed).uniform(-4.0, 4.0, n).astype(np.float32)


def render_session():
    """a 0.5 m map: a dense fan (key 0), a second one (key 1), key 2 missed, one-pixel keyframes (3, 4) that stretch the box;
    frames=[0] crops 15 x 9, which at twice the resolution is 7.5 x 4.5 -> 8 x 4: cvRound's tie upwards and downwards"""
    fan = SessionPing(33, 16, 0.25)
    b = _Builder("render_half", x0=-8.0, y0=-8.0, width=16.0, height=16.0, inc=4.0, resolution=0.5)
    b.add(0, (0.0, 0.0, 0.0), fan, _varied(8 * 33, 1))
    b.add(1, (-1.0, 0.5, 2.5), fan, _varied(8 * 33, 2))
    b.add(3, (5.25, 4.25, 0.0), PIXEL_PING, [2.5])
    b.add(4, (-5.25, -4.75, 0.0), PIXEL_PING, [-1.5])
    for frames in (None, [0], [1], [0, 3], [0, 4], [0, 2, 3, 99], [3], [2, 99], [1, 1, 0]):
        for f in RENDER_FACTORS:
            b.pub(frames=frames, resolution=0.5 * f)
    b.pub(frames=None, resolution=None).pub(frames=[0], resolution=0.0).pub(frames=[0], resolution=-1.0)
    return b.done()


def render_session_fifth():
    """a 0.2 m map published at 0.3: floor(i * inv) with inv = 1 / (0.2 / 0.3), which is not 1.5"""
    fan = SessionPing(17, 20, 0.2)
    b = _Builder("render_fifth", x0=-6.0, y0=-6.0, width=12.0, height=12.0, inc=4.0, resolution=0.2)
    b.add(0, (0.0, 0.0, 0.4), fan, _varied(20 * 17, 3))
    b.add(1, (0.5, -0.5, -1.0), fan, _varied(20 * 17, 4))
    for frames in (None, [0], [1]):
        for res in (0.3, 0.2, 0.218, 0.222, 0.4, 0.2 * 1.5):
            b.pub(frames=frames, resolution=res)
    return b.done()


def pixel_session():
    """a one-pixel geometry: the crop is 1 x 1; at twice the resolution cvRound(0.5) = 0 and the image is empty"""
    b = _Builder("render_1x1", x0=-4.0, y0=-4.0, width=8.0, height=8.0, inc=4.0, resolution=0.5)
    b.add(0, (0.25, 0.25, 0.0), PIXEL_PING, [1.25])
    for f in RENDER_FACTORS:
        b.pub(frames=None, resolution=0.5 * f).pub(frames=[0], resolution=0.5 * f)
    return b.done()


SATURATING = [20.0, -20.0, 40.0, -40.0, 104.0, -104.0, 1e38, -1e38, 88.0, -88.0]


def saturation_session():
    """log-odds large enough that expit is 1 in float32, or below 1e-8 and from -104 on exactly 0, added three times at one pose
    so that the sums reach +-312 and +-3e38 (finite in float32): every published cell is 0, 50 (never visited) or 100, and
    100 p is nowhere near another integer"""
    ping = SessionPing(9, 6, 0.5)
    b = _Builder("render_saturated", x0=-4.0, y0=-4.0, width=8.0, height=8.0, inc=4.0, resolution=0.5)
    lo = np.resize(np.array(SATURATING, np.float32), 6 * 9)
    for key in range(3):
        b.add(key, (0.1, 0.1, 0.2), ping, lo)
    for frames in (None, [0], [0, 1]):
        for f in (1.0, 2.0, 1.5):
            b.pub(frames=frames, resolution=0.5 * f)
    return b.done()


def render_sessions():
    return [render_session(), render_session_fifth(), pixel_session(), saturation_session()]


def info_of(msg):
    return [msg.info.origin.position.x, msg.info.origin.position.y, msg.info.width, msg.info.height, msg.info.resolution,
            msg.header.frame_id, msg.info.origin.orientation.w]


def clamp_never_binds(n, ratio):
    """whether the INTER_NEAREST source index floor(i * (1 / ratio)) stays below n for every output index: the clamp to
    n - 1 then changes nothing"""
    d = int(np.rint(n * ratio))
    return d == 0 or int(np.floor((d - 1) * (1.0 / ratio))) <= n - 1


# ---- what reference and product refuse alike --------------------------------------------------------------------------------
REFUSED_PINGS = [("one_beam", SessionPing(1, 8, 0.5), ValueError), ("three_beams", SessionPing(3, 8, 0.5), ValueError)]
REFUSED_RESOLUTIONS = [0.5 * 0.89, 0.25]     # of the 0.5 m render session: finer than the map by more than the 10 % gate
