"""numpy references for the keyed clouds of the 3-D keyframe store (sfe_store3.hip: put_keys, get_points_keys, fov_select,
compact_selected, match_keys) and the inputs their tests share, on top of tests/store3_ref.py and tests/pcl3_ref.py.

- ``get_points_keys``: ``transform_fma`` per cloud, a tag per point, np.concatenate, then ``pcl3_ref.downsample`` whose index
  output gathers the tags (the descriptor overload of pcl.downsample: a leaf's medoid brings its descriptor along).
- ``fov``: the gate of the loop-closure search, expression for expression ``store.fov3_numpy`` (float32 transform, norm,
  arctan2; float64 bounds), the union over the frames.  ``fov_margins`` adds a double-precision bearing per point / frame
  pair, by which the tests know how far every point is from its bound.
- ``compact``: boolean indexing.
- ``match_keys``: ``pcl3_ref.match`` plus np.bincount.
Test infrastructure only."""
import functools

import numpy as np

import icp3_cases as C
import pcl3_ref
import store3_ref as R

F = np.float32
TILE = 2048                                         # P3_TILE: target points per LDS tile of the matching kernels


def get_points_keys(clouds, Hs, keys, resolution):
    """-> (points N' x 3 float32, keys int32 [N'])"""
    parts = [R.transform_fma(c, H) for c, H in zip(clouds, Hs)]
    cat = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros((0, 3)), F).reshape(-1, 3)
    tags = np.concatenate([np.full(len(c), k, np.int32) for c, k in zip(clouds, keys)]) if parts else np.zeros(0, np.int32)
    tags = np.ascontiguousarray(tags, np.int32)
    if not resolution > 0 or len(cat) == 0:
        return cat, tags
    pts, idx = pcl3_ref.downsample(cat, resolution)
    return pts, tags[idx]


def range3(local):
    """sqrt(fl(fl(fl(x x) + fl(y y)) + fl(z z))): every operation a separate float32 numpy operation"""
    local = np.ascontiguousarray(local, F).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        xx, yy, zz = local[:, 0] * local[:, 0], local[:, 1] * local[:, 1], local[:, 2] * local[:, 2]
        return np.sqrt(((xx + yy).astype(F) + zz).astype(F)).astype(F)


def fov_frame(points, Hinv, range_bound, bearing_bound):
    """one frame of the gate: float32 transform (the fma chain), range, float32 arctan2; the bounds are float64"""
    local = R.transform_fma(points, Hinv)
    with np.errstate(invalid="ignore", over="ignore"):
        ranges = range3(local)
        bearings = np.arctan2(local[:, 1], local[:, 0])
        return (ranges < range_bound) & (abs(bearings) < bearing_bound)


def fov(points, Hinvs, range_bounds, bearing_bounds):
    """-> selection bytes uint8 [N]: the union over the frames"""
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    sel = np.zeros(len(points), bool)
    for H, rb, bb in zip(Hinvs, range_bounds, bearing_bounds):
        sel |= fov_frame(points, H, rb, bb)
    return sel.astype(np.uint8)


def fov_margins(points, Hinvs, range_bounds, bearing_bounds):
    """for every point / frame pair that passes the range test: (| |bearing| - bound |, |bearing|), the bearing in float64 from
    the float32 local point -> two float64 arrays"""
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    gaps, angles = [], []
    for H, rb, bb in zip(Hinvs, range_bounds, bearing_bounds):
        local = R.transform_fma(points, H)
        with np.errstate(invalid="ignore", over="ignore"):
            inside = range3(local).astype(np.float64) < rb
            a = np.abs(np.arctan2(local[:, 1].astype(np.float64), local[:, 0].astype(np.float64)))[inside]
        gaps.append(np.abs(a - bb))
        angles.append(a)
    if not gaps:
        return np.zeros(0), np.zeros(0)
    return np.concatenate(gaps), np.concatenate(angles)


def key_counts(keys, n_keys):
    """per-key counts of keys below n_keys (the others are not counted) -> int32 [n_keys]"""
    keys = np.asarray(keys, np.int64).reshape(-1)
    return np.bincount(keys[keys < n_keys], minlength=n_keys)[:n_keys].astype(np.int32)


def compact(points, keys, sel):
    sel = np.asarray(sel).astype(bool)
    return np.ascontiguousarray(points, F).reshape(-1, 3)[sel], np.asarray(keys, np.int32)[sel]


def match_keys(source, H, target, target_keys, max_dist, n_keys):
    """-> (per-key counts of the matched targets int32 [n_keys], number of matched source points)"""
    moved = R.transform_fma(source, H)
    target = np.ascontiguousarray(target, F).reshape(-1, 3)
    if len(moved) == 0 or len(target) == 0:
        return np.zeros(n_keys, np.int32), 0
    with np.errstate(invalid="ignore", over="ignore"):
        ids, d2 = pcl3_ref.match(target, moved, max_dist)
    ok = (ids[0] != -1) & (d2[0] < F(np.inf))
    hit = ids[0][ok]
    return key_counts(np.asarray(target_keys, np.int32)[hit], n_keys), int(ok.sum())


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
KEY_TOTALS = (1, 255, 256, 257, 2047, 2048, 2049, 4097)
FOV_SIZES = (63, 64, 65, 255, 256, 257)
COMPACT_SIZES = (1023, 1024, 1025, 2049)
MATCH_SOURCES = (1, 255, 256, 257)
MATCH_TARGETS = (2047, 2048, 2049, 4097)


@functools.lru_cache(maxsize=None)
def keyed_job(total):
    """up to three clouds that add up to ``total`` points, their motions and their keys (not in order, one repeated size)"""
    if total < 3:
        sizes = (total,)
    else:
        a = total // 3
        sizes = (a, 1, total - a - 1)
    clouds = [R.cloud(6000 + total + k, n, scale=(6.0, 6.0, 2.0)) for k, n in enumerate(sizes)]
    Hs = [R.motion(6100 + total + k, big=False) for k in range(len(sizes))]
    return clouds, Hs, [7, 2, 11][:len(sizes)]


@functools.lru_cache(maxsize=None)
def coincident_job():
    """two clouds that hold the same points (under the identity) with different keys, the second also a few of its own far
    away: every shared point has its twin in its leaf, and the medoid search keeps the first of two equal distances -- the
    earlier cloud's point -> (clouds, Hs, keys, resolution)"""
    a = (np.random.default_rng(61).integers(-40, 40, (300, 3)) * 0.25).astype(F)     # dyadic: the identity moves nothing
    a = np.unique(a, axis=0)
    b = np.concatenate([a[::-1], np.array([[100, 100, 100], [-100, 50, 25]], F)]).astype(F)
    return [a, b], [R.EYE, R.EYE], [5, 3], 0.1


@functools.lru_cache(maxsize=None)
def forty_keyed_jobs():
    """40 get_points_keys jobs of mixed sizes over the clouds of store3_ref.mixed_jobs, with keys
    -> (clouds, [(indices or -1, motions, keys)])"""
    clouds, jobs = R.mixed_jobs(40)
    rng = np.random.default_rng(62)
    return clouds, [(ids, Hs, [int(rng.integers(0, 50)) for _ in ids]) for ids, Hs in jobs]


def sensor_frame(seed, pos_scale=4.0):
    """a sensor pose (yaw about z, a small tilt, a position) -> the float32 4 x 4 of its inverse, as the gate takes it"""
    rng = np.random.default_rng(seed)
    P = C.rigid((0.02 * rng.normal(), 0.02 * rng.normal(), 1.0), rng.uniform(-np.pi, np.pi), rng.uniform(-1, 1, 3) * pos_scale)
    return np.asarray(np.linalg.inv(P), F)


@functools.lru_cache(maxsize=None)
def fov_case(n, n_frames, seed=0):
    """a keyed cloud of n points in a 40 x 40 x 6 m box and n_frames sensor frames with range bounds near 15 m and bearing
    bounds near 1.1 rad: every frame sees a good part of the cloud and misses a good part
    -> (points, keys, Hinvs, range_bounds, bearing_bounds)"""
    rng = np.random.default_rng(7000 + 13 * n + n_frames + 101 * seed)
    pts = (rng.uniform(-1, 1, (n, 3)) * np.array([20.0, 20.0, 3.0])).astype(F)
    keys = rng.integers(0, 12, n).astype(np.int32)
    Hinvs = [sensor_frame(7100 + 17 * n + 3 * f + seed) for f in range(n_frames)]
    rb = [float(15.0 + rng.uniform(0, 2)) for _ in range(n_frames)]
    bb = [float(1.1 + rng.uniform(0, 0.2)) for _ in range(n_frames)]
    return pts, keys, Hinvs, rb, bb


@functools.lru_cache(maxsize=None)
def fov_special():
    """Under the identity, on dyadic coordinates (transform and squares exact), one frame with range bound 5.0 and bearing
    bound 2.0: a range exactly on its bound (strict test: not selected), the float below it (selected), the origin
    (range 0, bearing 0: selected), points behind the sensor (bearing pi or -pi: not selected), NaN and infinite points
    (never selected), keys at and above n_keys = 4 (selected, not counted)
    -> (points, keys, Hinvs, range_bounds, bearing_bounds, expected selection, n_keys)"""
    below = np.nextafter(F(5.0), F(0))
    pts = np.array([[3, 0, 4],               # range 5.0 = the bound: not selected
                    [below, 0, 0],           # the float below: selected
                    [0, 0, 0],               # the origin: selected
                    [-1, 0, 0],              # bearing +pi
                    [-1, -2.0 ** -100, 0],   # bearing -pi (a -0.0 would not survive the transform's "+ 0")
                    [-2, 0, 1],
                    [np.nan, 0, 0], [0, np.nan, 0], [0, 0, np.nan],
                    [np.inf, 0, 0], [0, -np.inf, 0], [1, 1, np.inf],
                    [1, 1, 1],               # key 4 = n_keys: selected, not counted
                    [1, -1, 2],              # key 9: selected, not counted
                    [0, 3, 0],               # bearing pi / 2 < 2: selected
                    [0, 0, 4.5]], F)         # straight up: range by z alone, bearing atan2(0, 0) = 0: selected
    keys = np.array([0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3, 4, 9, 3, 3], np.int32)
    want = np.array([0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1], np.uint8)
    return pts, keys, [R.EYE], [5.0], [2.0], want, 4


@functools.lru_cache(maxsize=None)
def fov_on_the_bearing_bound():
    """a cloud of 200 points with one whose double-precision bearing is, to within 1e-9 relative, the frame's bearing bound:
    the device cannot decide it (its margin is 1e-6 relative) -> (points, keys, Hinvs, range_bounds, bearing_bounds, index)"""
    pts, keys, Hinvs, rb, bb = fov_case(200, 1, seed=5)
    pts = pts.copy()
    pts[77] = (3.0, 2.0, 0.5)
    local = R.transform_fma(pts[77:78], Hinvs[0])
    bound = float(abs(np.arctan2(np.float64(local[0, 1]), np.float64(local[0, 0]))))
    assert float(range3(local)[0]) < rb[0]
    return pts, keys, Hinvs, rb, [bound], 77


@functools.lru_cache(maxsize=None)
def selection(n, kind, seed=0):
    """a selection over n points: "none", "all", or about half ("half"); "survivors:<m>" selects exactly m points"""
    rng = np.random.default_rng(8000 + n + seed)
    if kind == "none":
        return np.zeros(n, np.uint8)
    if kind == "all":
        return np.ones(n, np.uint8)
    if kind == "half":
        return (rng.uniform(size=n) < 0.5).astype(np.uint8)
    m = int(kind.split(":")[1])
    sel = np.zeros(n, np.uint8)
    sel[rng.permutation(n)[:m]] = 1
    return sel


@functools.lru_cache(maxsize=None)
def match_pair(ns, nt):
    """store3_ref.overlap_pair with keys on the target -> (source, H, target, target keys, max_dist)"""
    src, H, tgt, max_dist = R.overlap_pair(ns, nt)
    keys = np.random.default_rng(9000 + ns + nt).integers(0, 20, nt).astype(np.int32)
    return src, H, tgt, keys, max_dist


@functools.lru_cache(maxsize=None)
def tie_case():
    """Under the identity, on dyadic coordinates.  A target of 2 TILE + 3 points, all far away except the ones placed below,
    and five sources, each at exactly the same float distance from two targets with DIFFERENT keys:
      source 0: targets 5 and 9               (inside the first tile)
      source 1: targets TILE - 1 and TILE     (across the first tile border)
      source 2: targets 100 and 2 TILE + 1    (two tiles apart)
      source 3: targets TILE + 7 and 2 TILE   (across the second border)
      source 4: targets 2 TILE + 2 and 3      (the later tile's point is listed first here; the lower index still wins)
    -> (source, target, target keys, max_dist, [(lower index, higher index) per source])"""
    nt = 2 * TILE + 3
    tgt = np.zeros((nt, 3), F)
    tgt[:, 0] = 1000.0 + np.arange(nt)                  # far from every source
    keys = (np.arange(nt) % 5).astype(np.int32)
    pairs = [(5, 9), (TILE - 1, TILE), (100, 2 * TILE + 1), (TILE + 7, 2 * TILE), (3, 2 * TILE + 2)]
    src = np.zeros((len(pairs), 3), F)
    for s, (lo, hi) in enumerate(pairs):
        c = np.array([16.0 * s, -8.0, 4.0], F)
        src[s] = c
        tgt[lo] = c + np.array([0.5, 0, 0], F)          # d2 = 0.25 on both sides, by different coordinates
        tgt[hi] = c + np.array([0, 0, -0.5], F)
        keys[lo], keys[hi] = 10 + s, 20 + s
    return src, tgt, keys, 1.0, pairs


@functools.lru_cache(maxsize=None)
def radius_case():
    """store3_ref.boundary_case with keys: d2 exactly r2 is matched, the next float above is not, NaN and infinite sources never
    -> (source, target, target keys, max_dist, expected overlap, expected per-key counts for n_keys = 2)"""
    src, tgt, max_dist, want = R.boundary_case()
    # ... and a source whose d2 = 0.5625 + 2^-24 is exactly the float above r2 (both squares and the sum are exact)
    src = np.concatenate([src, np.array([[0.75, 2.0 ** -12, 0]], F)])
    keys = np.array([0, 1, 5], np.int32)                # (the third target: matched by nobody)
    return src, tgt, keys, max_dist, want, np.array([2, 1], np.int32)


# ---- a small session with a loop -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def loop_session():
    """twelve keyframes of 300 .. 800 points of one world along a path that comes back to its start
    -> (frames float32 in their own sensor frames, poses float64 4 x 4)"""
    rng = np.random.default_rng(12)
    world = rng.uniform(-1, 1, (6000, 3)) * np.array([14.0, 14.0, 2.0])
    poses, frames = [], []
    for k in range(12):
        th = 2 * np.pi * k / 11.0                        # keyframe 11 is back where keyframe 0 was
        centre = np.array([6.0 * np.cos(th), 6.0 * np.sin(th), 0.1 * np.sin(3 * th)])
        P = C.rigid((0.01, -0.02, 1.0), th + np.pi / 2, centre)
        Pi = np.linalg.inv(P)
        local = C.apply(Pi, world)
        seen = np.nonzero((np.linalg.norm(local, axis=1) < 11.0) & (np.abs(np.arctan2(local[:, 1], local[:, 0])) < 1.0))[0]
        n = min(len(seen), 300 + (k * 137) % 501)
        pick = rng.permutation(seen)[:n]
        frames.append((local[pick] + rng.normal(0, 0.004, (n, 3))).astype(F))
        poses.append(P)
    return frames, poses


LOOP = dict(min_st_sep=4, resolution=0.3, max_range=12.0, aperture=2.2, range_std=0.1, bearing_std=0.02, max_dist=0.5)


def loop_frames_bounds(source_frames):
    """per source frame of the loop session: (inverse pose float32 4 x 4, range bound, bearing bound), as slam.py:881-888
    forms them (here from fixed standard deviations)"""
    _, poses = loop_session()
    Hinvs = [np.asarray(np.linalg.inv(poses[f]), F) for f in source_frames]
    rb = [LOOP["range_std"] * (1 + 0.1 * k) * 5.0 + LOOP["max_range"] for k in range(len(source_frames))]
    bb = [LOOP["bearing_std"] * (1 + 0.1 * k) * 5.0 + LOOP["aperture"] * 0.5 for k in range(len(source_frames))]
    return Hinvs, rb, bb


LOOP_SOURCE_FRAMES = (11, 10)
LOOP_TARGET_FRAMES = tuple(range(12 - LOOP["min_st_sep"]))


@functools.lru_cache(maxsize=None)
def loop_target():
    """the keyed target of the loop session: keyframes 0 .. 7 in the global frame, tagged with their index, downsampled"""
    frames, poses = loop_session()
    return get_points_keys([frames[k] for k in LOOP_TARGET_FRAMES], [np.asarray(poses[k], F) for k in LOOP_TARGET_FRAMES],
                           list(LOOP_TARGET_FRAMES), LOOP["resolution"])


@functools.lru_cache(maxsize=None)
def planar_session():
    """five keyframes with z = 0 under planar poses: what the 2-D store holds as (x, y) -> (frames N x 3, poses 4 x 4 float64)"""
    rng = np.random.default_rng(21)
    world = np.c_[rng.uniform(-1, 1, (1500, 2)) * 12.0, np.zeros(1500)]
    frames, poses = [], []
    for k in range(5):
        P = C.planar_motion(1.5 * k, -0.8 * k, 0.4 * k)
        local = C.apply(np.linalg.inv(P), world)
        pick = rng.permutation(len(world))[:200 + 37 * k]
        frames.append(np.ascontiguousarray(local[pick], F))
        frames[-1][:, 2] = 0
        poses.append(np.asarray(P, np.float64))
    return frames, poses


def gate_inputs():
    """(points, Hinvs, range bounds, bearing bounds) of every gate the GPU tests run, except the one built to sit on its
    bearing bound (fov_on_the_bearing_bound)"""
    for n in FOV_SIZES:
        p, _, H, rb, bb = fov_case(n, 2)
        yield p, H, rb, bb
    p, _, H, rb, bb = fov_case(500, 3)
    yield p, H, rb, bb
    for k, n in enumerate(FOV_MULTI):
        p, _, H, rb, bb = fov_case(n, 1 + k % 3, seed=1)
        yield p, H, rb, bb
    p, _, H, rb, bb, _, _ = fov_special()
    yield p, H, rb, bb
    frames, poses = planar_session()
    tp, _ = get_points_keys(frames[:3], [np.asarray(P, F) for P in poses[:3]], [0, 1, 2], 0.25)
    yield tp, [np.asarray(np.linalg.inv(poses[4]), F)], [14.0], [1.2]
    tp, _ = loop_target()
    H, rb, bb = loop_frames_bounds(LOOP_SOURCE_FRAMES)
    yield tp, H, rb, bb


FOV_MULTI = (700, 1, 256, 0, 1025, 64)      # clouds of one call: blocks of the smaller ones leave whole
