"""Times of the device occupancy map (sonar_slam_amd.mapping) next to the numpy restatement of the reference
(tests/mapping_ref.py) on the same synthetic session: 1024 ranges x 512 beams at 30 m, the shipped 0.2 m map resolution.
Prints one JSON line:
  add_keyframe_ms        per add_keyframe from points (outlier filter, measurement, fit, add)
  update_poses_ms        update_poses with K = 100 and K = 1000 keyframes all changed (device: one call; numpy: the
                         update_pose loop of the reference)
  render_ms              get_occupancy_grid1() over the whole box (about 1000 x 1000 cells)
The numpy side adds only `--ref-adds` keyframes from points (the rest through add_keyframe_logodds, which skips the
measurement) to keep the run short.

With `--sessions S` (default 32; 0 skips the leg) also the lock-step map, under "lockstep": a MapBatch of S sessions next
to S looped Mapping objects on the same inputs (session s is the session above, shifted by s metres), both in this process,
alternated call by call, the median of the repetitions:
  add_keyframes_ms       one add_keyframes call for S sessions / S add_keyframe calls, over `--batch-keyframes` steps
  update_poses_ms        one update_poses call that moves every keyframe of every session / S update_poses calls,
                         `--reps` times (the poses alternate between two sets)
  ratio                  looped / lock-step

With `--feed host|store` only the map feed of a lock-step session is timed, under "feed": what chained.SessionBatch does at
the end of every step for S sessions whose keyframe clouds lie in a CloudStore -- `host`: store.read_many + add_keyframes
(the clouds cross to the host and back), `store`: add_keyframes_store (they stay on the device) -- over `--batch-keyframes`
steps, the first left out:
  step_ms                the median per step, host synchronised
  points, undecided      points fed, and those the device left to the host (store feed)
  readbacks_per_step     host read-backs of the measurement per step (the fit's bounds come on top on both routes)
  grid_sha               sha256 of every session's final grid: equal between the two feeds

With `--feed store` and no `--sessions` (or `--sessions 0`) the feed of a single Mapping, under "feed_single": three
Mappings on the same session in this process, alternated keyframe by keyframe over `--batch-keyframes` keyframes, the first
left out -- `add_keyframe` on clouds that are already on the host, `store.read` + `add_keyframe` (what a node whose
clouds lie in a CloudStore has to do without the store feed), and `add_keyframe_store`:
  add_keyframe_ms        the median per add of each route, host synchronised
  undecided_share        points the device left to the host / points fed
  readbacks_per_add      host read-backs of the measurement per add (the fit's bounds come on top on every route)
  grids_equal            the three final grids are bit for bit equal

With `--method 2` only the point-projection map is timed, under "method2": a Mapping of `--batch-keyframes` keyframes with
its keyed SLAM cloud (every keyframe's 300 points registered with its pose: float32 x, y, 0, key), fed with pub_occupancy1
off, and -- with `--sessions S` > 0 -- a MapBatch of S such sessions (session s shifted by s metres):
  get_occupancy_grid2_ms one call, the whole map and `frames` = the last 10 keyframes at 0.5 m: the device route (host
                         selection and plan, one sfe_map_render2 call, read-back) next to the numpy restatement
                         tests/mapping2_ref.py on the cell lists read back beforehand (its filter is the C oracle's), the
                         median of `--reps` alternated repetitions
  lockstep               one MapBatch.get_occupancy_grid2 call for all S sessions; `numpy_one_session_ms` is the restatement
                         for one of them
  images_equal           the device images equal the restatement's

With `--method 2 --feed store` the store route of method 2 is timed next to the host route, under "method2_store": the
same map, its keyed SLAM cloud in a CloudStore (put_keys), both routes in this process, alternated call by call, the median
of `--reps` repetitions (`--feed host`: the host leg alone):
  host                   what a caller has to do today: store.read + store.read_keys, the (N, 4) cloud, select_points on the
                         host, get_occupancy_grid2 (upload of float64 pairs, render, read-back)
  store                  get_occupancy_grid2_store: the cloud stays where it is
  lockstep               with `--sessions S` > 0: one MapBatch call for all S sessions by each route
  images_equal           both routes give the same images

With `--intensity` only the intensity mosaic (pub_intensity with intensity_skips="oculus") is timed, under "intensity": two
Mappings on the same session and pings in this process, the mosaic on and off, alternated call by call:
  add_keyframe_ms        the median per add_keyframe from points over `--keyframes` keyframes: on, off, and the numpy
                         restatement tests/intensity_ref.py (its first `--ref-adds` adds)
  update_poses_ms        one update_poses call that moves all `--keyframes` keyframes, `--reps` alternated repetitions: on,
                         off, and the restatement's update_pose loop (once)
  render_ms              get_intensity_grid() over the whole box, device and numpy; images_equal
  lockstep_feed          with `--sessions S` > 0: one add_keyframes call for S sessions over `--batch-keyframes` steps, two
                         MapBatches alternated: `device` takes the S pings where they lie on the device (what
                         chained.SessionBatch feeds from its resident frames), `host` the same pings as a host array (one
                         upload of S pings per step); `off` is the same call without the mosaic

    python tools/mapping_times.py [--keyframes 1000] [--ref-adds 20] [--sessions 32] [--batch-keyframes 40] [--reps 5]
    python tools/mapping_times.py --sessions 32 --feed store
    python tools/mapping_times.py --feed store --batch-keyframes 200
    python tools/mapping_times.py --method 2 --sessions 32
    python tools/mapping_times.py --method 2 --feed store --sessions 32
    python tools/mapping_times.py --intensity --sessions 32
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import intensity_ref  # noqa: E402
import mapping2_ref  # noqa: E402
import mapping_ref  # noqa: E402
import oracle  # noqa: E402
from sonar_slam_amd import _lib  # noqa: E402
from sonar_slam_amd.mapping import DeviceImage, MapBatch, Mapping  # noqa: E402
from sonar_slam_amd.pose2 import Pose2  # noqa: E402


def session(n, seed=5):
    rng = np.random.default_rng(seed)
    poses, clouds = [], []
    x = y = th = 0.0
    for k in range(n):
        # a lawnmower over about 180 m x 180 m
        lane, along = divmod(k, 100)
        x = -90.0 + 1.8 * along if lane % 2 == 0 else 90.0 - 1.8 * along
        y = -90.0 + 18.0 * lane
        th = 0.0 if lane % 2 == 0 else np.pi
        th += rng.normal(0, 0.02)
        poses.append((x, y, th))
        b = np.r_[rng.uniform(-1.0, -0.3, 150), rng.uniform(0.2, 0.9, 150)]
        rho = np.r_[rng.uniform(12, 14, 150), rng.uniform(20, 24, 150)]
        clouds.append(np.c_[rho * np.cos(b), rho * np.sin(b)].astype(np.float32).astype(np.float64))
    return poses, clouds


def timed(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def lockstep(ctx, ping, settings, S, K, reps):
    """MapBatch of S sessions against S looped Mappings, alternated in one process -> the "lockstep" record"""
    poses, clouds = session(K)
    pose = lambda s, k, d=0.0: Pose2(poses[k][0] + s + d, poses[k][1] - d, poses[k][2] + 0.01 * d)
    batch = MapBatch(ctx, S, K, **settings)
    batch.configure()
    loop = []
    for _ in range(S):
        m = Mapping(ctx)
        for k, v in settings.items():
            setattr(m, k, v)
        m.configure()
        loop.append(m)
    sessions = list(range(S))

    def add_batch(k):
        batch.add_keyframes(sessions, [k] * S, [pose(s, k) for s in sessions], ping, [clouds[k]] * S)
        ctx.sync()

    def add_loop(k):
        for s in sessions:
            loop[s].add_keyframe(k, pose(s, k), ping, clouds[k])
        ctx.sync()
    t_b, t_l = [], []
    for k in range(K):
        first, second = (add_batch, add_loop) if k % 2 == 0 else (add_loop, add_batch)
        a, b = timed(lambda: first(k)), timed(lambda: second(k))
        if k:                       # step 0: geometry upload, first allocations
            (t_b if first is add_batch else t_l).append(a)
            (t_l if first is add_batch else t_b).append(b)
    flat_s = [s for k in range(K) for s in sessions]
    flat_k = [k for k in range(K) for s in sessions]
    u_b, u_l = [], []
    for rep in range(reps + 1):
        d = 0.7 if rep % 2 == 0 else 0.0
        flat_p = [pose(s, k, d) for k in range(K) for s in sessions]
        keys_s = list(range(K))
        poses_s = [[pose(s, k, d) for k in range(K)] for s in sessions]      # both legs get their poses ready-made

        def up_batch():
            batch.update_poses(flat_s, flat_k, flat_p)
            ctx.sync()

        def up_loop():
            for s in sessions:
                loop[s].update_poses(keys_s, poses_s[s])
            ctx.sync()
        first, second = (up_batch, up_loop) if rep % 2 == 0 else (up_loop, up_batch)
        a, b = timed(first), timed(second)
        if rep:                     # the first pass grows scratch buffers
            (u_b if first is up_batch else u_l).append(a)
            (u_l if first is up_batch else u_b).append(b)
    equal = all(np.array_equal(batch.maps[s].logodds_grid.view(np.int32), loop[s].logodds_grid.view(np.int32))
                for s in (0, S - 1))
    med = lambda v: float(np.median(v))
    out = {"sessions": S, "keyframes": K, "reps": reps, "apply_rounds": batch.last_apply_rounds,
           "add_keyframes_ms": {"lockstep": med(t_b), "looped": med(t_l), "ratio": med(t_l) / med(t_b)},
           "update_poses_ms": {"lockstep": med(u_b), "looped": med(u_l), "ratio": med(u_l) / med(u_b)},
           "grids_equal": bool(equal)}
    batch.close()
    for m in loop:
        m.close()
    return out


def feed(ctx, ping, settings, S, K, route):
    """the per-step map feed of S sessions from a CloudStore by one route -> the "feed" record"""
    import hashlib
    from sonar_slam_amd.store import CloudStore
    poses, clouds = session(K)
    pose = lambda s, k: Pose2(poses[k][0] + s, poses[k][1], poses[k][2])
    store = CloudStore(ctx, capacity_points=S * K * 512, max_clouds=S * K)
    # session s sees the session's cloud turned a little, so that no two clouds are equal
    handles = np.array([[store.put(clouds[k].dot(np.array([[np.cos(0.002 * s), np.sin(0.002 * s)],
                                                            [-np.sin(0.002 * s), np.cos(0.002 * s)]])))
                         for k in range(K)] for s in range(S)], np.int32)
    batch = MapBatch(ctx, S, K, **settings)
    batch.configure()
    sessions = list(range(S))
    times, und = [], 0
    for k in range(K):
        args = (sessions, [k] * S, [pose(s, k) for s in sessions], ping)

        def step():
            if route == "store":
                batch.add_keyframes_store(*args, store, handles[:, k])
            else:
                batch.add_keyframes(*args, store.read_many(handles[:, k]))
            ctx.sync()
        before = batch.feed_stats["undecided"]
        t = timed(step)
        und += batch.feed_stats["undecided"] > before
        if k:                       # step 0: geometry upload, first allocations
            times.append(t)
    h = hashlib.sha256()
    for v in batch.maps:
        h.update(v.logodds_grid.tobytes())
    stats = batch.feed_stats
    if route == "store":
        # the undecided counters every step, the undecided points on the steps that have some
        readbacks = 1.0 + und / float(K)
    else:
        readbacks = 2.0             # the clouds (read_many), the keep flags of the outlier filter
    out = {"route": route, "sessions": S, "steps": K, "step_ms": float(np.median(times)), "step_ms_min": float(np.min(times)),
           "points": int(store.counts(handles.ravel()).sum()), "undecided": stats["undecided"], "fed_points": stats["points"],
           "readbacks_per_step": readbacks, "grid_sha": h.hexdigest()}
    batch.close()
    store.close()
    return out


def feed_single(ctx, ping, settings, K):
    """one Mapping fed by add_keyframe (host clouds), store.read + add_keyframe, and add_keyframe_store -> the "feed_single" record"""
    from sonar_slam_amd.store import CloudStore
    poses, clouds = session(K)
    store = CloudStore(ctx, capacity_points=K * 512, max_clouds=K)
    handles = [store.put(c) for c in clouds]
    host32 = [store.read(h) for h in handles]          # what add_keyframe is handed on the host route
    maps = {}
    for name in ("host", "read_back", "store"):
        m = Mapping(ctx)
        for k, v in settings.items():
            setattr(m, k, v)
        m.configure()
        maps[name] = m
    add = {"host": lambda k, p: maps["host"].add_keyframe(k, p, ping, host32[k]),
           "read_back": lambda k, p: maps["read_back"].add_keyframe(k, p, ping, store.read(handles[k])),
           "store": lambda k, p: maps["store"].add_keyframe_store(k, p, ping, store, handles[k])}
    times = {name: [] for name in add}
    names, und = list(add), 0
    for k in range(K):
        p = Pose2(*poses[k])
        before = maps["store"].feed_stats["undecided"]
        for name in names[k % 3:] + names[:k % 3]:
            t = timed(lambda: (add[name](k, p), ctx.sync()))
            if k:                   # keyframe 0: geometry upload, first allocations
                times[name].append(t)
        und += maps["store"].feed_stats["undecided"] > before
    grids = [m.logodds_grid for m in maps.values()]
    stats = maps["store"].feed_stats
    out = {"keyframes": K, "image": list(maps["store"].oculus_image_size),
           "add_keyframe_ms": {name: float(np.median(t)) for name, t in times.items()},
           "add_keyframe_ms_min": {name: float(np.min(t)) for name, t in times.items()},
           "points": stats["points"], "undecided": stats["undecided"],
           "undecided_share": stats["undecided"] / float(max(stats["points"], 1)),
           # host: the keep flags of the outlier filter; read_back: the cloud on top; store: the undecided counter every
           # add, the undecided points on the adds that have some
           "readbacks_per_add": {"host": 1.0, "read_back": 2.0, "store": 1.0 + und / float(K)},
           "grids_equal": bool(all(np.array_equal(grids[0].view(np.int32), g.view(np.int32)) for g in grids[1:]))}
    for m in maps.values():
        m.close()
    store.close()
    return out


def method2(ctx, ping, settings, S, K, reps):
    """get_occupancy_grid2 of one Mapping, and of a MapBatch of S sessions, next to the numpy restatement -> the "method2" record"""
    poses, clouds = session(K)

    def keyed(shift):
        parts = []
        for k, ((x, y, th), pts) in enumerate(zip(poses, clouds)):
            c, s = np.cos(th), np.sin(th)
            g = np.c_[c * pts[:, 0] - s * pts[:, 1] + x + shift, s * pts[:, 0] + c * pts[:, 1] + y]
            parts.append(np.c_[g, np.zeros(len(g)), np.full(len(g), float(k))])
        return np.concatenate(parts).astype(np.float32)
    settings = dict(settings, pub_occupancy1=False)
    m = Mapping(ctx)
    for k, v in settings.items():
        setattr(m, k, v)
    m.configure()
    cloud = keyed(0.0)
    for k in range(K):
        m.add_keyframe(k, Pose2(*poses[k]), ping, cloud)
    cells = [(kf.r, kf.c) for kf in m.keyframes]
    queries = {"all": dict(), "last10_coarse": dict(frames=list(range(max(0, K - 10), K)), resolution=0.5)}
    med = lambda v: float(np.median(v))
    out = {"keyframes": K, "points": len(cloud), "dilate_size": int(m.dilate_size), "reps": reps, "get_occupancy_grid2_ms": {}}
    equal = True
    for name, kw in queries.items():
        t_d, t_n = [], []
        for rep in range(reps + 1):
            got, want = [None], [None]
            dev = lambda: got.__setitem__(0, m.get_occupancy_grid2(**kw))
            ref = lambda: want.__setitem__(0, mapping2_ref.occupancy_grid2(m, cells, cloud, oracle.remove_outlier, **kw))
            first, second = (dev, ref) if rep % 2 == 0 else (ref, dev)
            a, b = timed(first), timed(second)
            if rep:                 # the first call grows the scratch
                (t_d if first is dev else t_n).append(a)
                (t_n if first is dev else t_d).append(b)
            equal = equal and np.array_equal(got[0].occ, want[0]["data"])
        out["get_occupancy_grid2_ms"][name] = {"device": med(t_d), "numpy": med(t_n), "image": list(got[0].occ.shape),
                                               "selected_points": len(want[0]["points"]), "kept": want[0]["kept"]}
    if S > 0:
        batch = MapBatch(ctx, S, K, **settings)
        batch.configure()
        sessions = list(range(S))
        shifted = [keyed(float(s)) for s in sessions]
        for k in range(K):
            batch.add_keyframes(sessions, [k] * S, [Pose2(poses[k][0] + s, poses[k][1], poses[k][2]) for s in sessions], ping,
                                shifted)
        out["lockstep"] = {"sessions": S}
        for name, kw in queries.items():
            t_b = [timed(lambda: batch.get_occupancy_grid2(**kw)) for _ in range(reps + 1)][1:]
            v = batch.maps[S - 1]
            last = [(kf.r, kf.c) for kf in v.keyframes]
            t_n = [timed(lambda: mapping2_ref.occupancy_grid2(v, last, shifted[S - 1], oracle.remove_outlier, **kw))
                   for _ in range(max(1, reps // 2))]
            want = mapping2_ref.occupancy_grid2(v, last, shifted[S - 1], oracle.remove_outlier, **kw)
            equal = equal and np.array_equal(batch.get_occupancy_grid2(**kw)[S - 1].occ, want["data"])
            out["lockstep"][name] = {"lockstep_ms": med(t_b), "numpy_one_session_ms": med(t_n),
                                     "numpy_all_sessions_ms": med(t_n) * S}
        batch.close()
    out["images_equal"] = bool(equal)
    m.close()
    return out


def method2_store(ctx, ping, settings, S, K, reps, routes):
    """get_occupancy_grid2 of a cloud that lies in a CloudStore, by the host route and the store route -> the "method2_store"
    record"""
    from sonar_slam_amd.store import CloudStore
    poses, clouds = session(K)

    def keyed(shift):
        parts = []
        for k, ((x, y, th), pts) in enumerate(zip(poses, clouds)):
            c, s = np.cos(th), np.sin(th)
            g = np.c_[c * pts[:, 0] - s * pts[:, 1] + x + shift, s * pts[:, 0] + c * pts[:, 1] + y]
            parts.append(np.c_[g, np.zeros(len(g)), np.full(len(g), float(k))])
        return np.concatenate(parts).astype(np.float32)

    def read_back(h):
        pts = store.read(h)
        return np.c_[pts, np.zeros(len(pts)), store.read_keys(h)].astype(np.float32)
    settings = dict(settings, pub_occupancy1=False)
    store = CloudStore(ctx, capacity_points=(max(S, 0) + 1) * K * 320, max_clouds=max(S, 0) + 2)
    m = Mapping(ctx)
    for k, v in settings.items():
        setattr(m, k, v)
    m.configure()
    cloud = keyed(0.0)
    for k in range(K):
        m.add_keyframe(k, Pose2(*poses[k]), ping, cloud)
    handle = store.put_keys(cloud[:, :2], cloud[:, 3])
    queries = {"all": dict(), "last10_coarse": dict(frames=list(range(max(0, K - 10), K)), resolution=0.5)}
    med = lambda v: float(np.median(v))
    out = {"keyframes": K, "points": len(cloud), "reps": reps, "routes": list(routes), "get_occupancy_grid2_ms": {}}
    equal = True

    def alternate(legs):
        """-> ({route: times without the first round}, {route: last result})"""
        times, last = {r: [] for r in legs}, {}
        names = list(legs)
        for rep in range(reps + 1):
            for r in names[rep % len(names):] + names[:rep % len(names)]:
                t = time.perf_counter()
                last[r] = legs[r]()
                if rep:             # the first call grows the scratch
                    times[r].append((time.perf_counter() - t) * 1e3)
        return times, last

    def one_host(kw):
        m.point_cloud = read_back(handle)
        return m.get_occupancy_grid2(**kw)
    for name, kw in queries.items():
        legs = {"host": lambda: one_host(kw), "store": lambda: m.get_occupancy_grid2_store(store, handle, **kw)}
        times, last = alternate({r: legs[r] for r in routes})
        if len(routes) == 2:
            equal = equal and np.array_equal(last["host"].occ, last["store"].occ)
        rec = {r: med(times[r]) for r in routes}
        rec.update({r + "_min": float(np.min(times[r])) for r in routes})
        rec["image"] = list(last[routes[0]].occ.shape)
        if len(routes) == 2:
            rec["host_over_store"] = rec["host"] / rec["store"]
        out["get_occupancy_grid2_ms"][name] = rec
    if S > 0:
        batch = MapBatch(ctx, S, K, **settings)
        batch.configure()
        sessions = list(range(S))
        shifted = [keyed(float(s)) for s in sessions]
        for k in range(K):
            batch.add_keyframes(sessions, [k] * S, [Pose2(poses[k][0] + s, poses[k][1], poses[k][2]) for s in sessions], ping,
                                shifted)
        handles = [store.put_keys(c[:, :2], c[:, 3]) for c in shifted]
        out["lockstep"] = {"sessions": S}
        for name, kw in queries.items():
            legs = {"host": lambda: batch.get_occupancy_grid2(point_clouds=[read_back(h) for h in handles], **kw),
                    "store": lambda: batch.get_occupancy_grid2_store(store, handles, **kw)}
            times, last = alternate({r: legs[r] for r in routes})
            if len(routes) == 2:
                equal = equal and all(np.array_equal(a.occ, b.occ) for a, b in zip(last["host"], last["store"]))
            rec = {r: med(times[r]) for r in routes}
            rec.update({r + "_min": float(np.min(times[r])) for r in routes})
            if len(routes) == 2:
                rec["host_over_store"] = rec["host"] / rec["store"]
            out["lockstep"][name] = rec
        batch.close()
    if len(routes) == 2:
        out["images_equal"] = bool(equal)
    m.close()
    store.close()
    return out


def intensity(ctx, ping, settings, n, ref_adds, S, K, reps):
    """the intensity mosaic on against off, the numpy restatement, and the lock-step feed from device pings against host
    pings -> the "intensity" record"""
    poses, clouds = session(n)
    rng = np.random.default_rng(11)
    images = [rng.integers(0, 256, (ping.num_ranges, len(ping.bearings)), dtype=np.uint8) for _ in range(8)]
    on_settings = dict(settings, pub_intensity=True, intensity_skips="oculus")
    maps = {}
    for name, st in (("on", on_settings), ("off", settings)):
        m = Mapping(ctx)
        for k, v in st.items():
            setattr(m, k, v)
        m.configure()
        maps[name] = m
    ref = intensity_ref.Mapping()
    ref.remove_outlier = oracle.remove_outlier
    for k, v in settings.items():
        setattr(ref, k, v)
    ref.configure()
    add = {"on": lambda k: maps["on"].add_keyframe(k, Pose2(*poses[k]), ping, clouds[k], image=images[k % 8]),
           "off": lambda k: maps["off"].add_keyframe(k, Pose2(*poses[k]), ping, clouds[k])}
    t_add = {"on": [], "off": []}
    for k in range(n):
        for name in (("on", "off") if k % 2 == 0 else ("off", "on")):
            t = timed(lambda: (add[name](k), ctx.sync()))
            if k:                   # keyframe 0: geometry upload, first allocations
                t_add[name].append(t)
    t_ref = []
    for k in range(n):
        if k < ref_adds:
            t_ref.append(timed(lambda: ref.add_keyframe(k, Pose2(*poses[k]), ping, clouds[k], image=images[k % 8])))
        else:
            ref.add_keyframe_logodds(k, Pose2(*poses[k]), ping, maps["on"].keyframes[k].logodds, image=images[k % 8])
    med = lambda v: float(np.median(v))
    out = {"keyframes": n, "image": list(maps["on"].oculus_image_size), "reps": reps,
           "add_keyframe_ms": {"on": med(t_add["on"]), "off": med(t_add["off"]), "numpy": med(t_ref),
                               "on_min": float(np.min(t_add["on"])), "off_min": float(np.min(t_add["off"]))}}
    t_up = {"on": [], "off": []}
    keys = list(range(n))
    for r in range(reps + 1):
        d = 0.7 if r % 2 == 0 else 0.0
        new = [Pose2(poses[k][0] + d, poses[k][1] - d, poses[k][2] + 0.01 * d) for k in keys]
        for name in (("on", "off") if r % 2 == 0 else ("off", "on")):
            t = timed(lambda: (maps[name].update_poses(keys, new), ctx.sync()))
            if r:                   # the first pass grows scratch buffers
                t_up[name].append(t)
        if r == 0:
            def ref_loop():
                for k in keys:
                    ref.update_pose(k, new[k])
            t_up["numpy"] = [timed(ref_loop)]
    out["update_poses_ms"] = {name: med(v) for name, v in t_up.items()}
    out["update_poses_ms"].update({name + "_min": float(np.min(t_up[name])) for name in ("on", "off")})
    # (the restatement made the first move only: bring it to the maps' last poses before comparing)
    if reps % 2 == 1:
        for k in keys:
            ref.update_pose(k, Pose2(*poses[k]))
    maps["on"].get_intensity_grid()
    rd = [timed(maps["on"].get_intensity_grid) for _ in range(3)]
    rr = [timed(ref.get_intensity_grid) for _ in range(3)]
    got, want = maps["on"].get_intensity_grid(), ref.get_intensity_grid()
    out["render_ms"] = {"device": med(rd), "numpy": med(rr), "box": list(got.occ.shape)}
    out["images_equal"] = bool(got.occ.shape == want.occ.shape and np.array_equal(got.occ, want.occ))
    out["grids_equal"] = bool(np.array_equal(maps["on"].intensity_grid, ref.intensity_grid) and
                              np.array_equal(maps["on"].counter_grid, ref.counter_grid) and
                              np.array_equal(maps["on"].logodds_grid.view(np.int32), maps["off"].logodds_grid.view(np.int32)))
    for m in maps.values():
        m.close()
    if S > 0:
        rows, cols = images[0].shape
        frames = np.stack([images[s % 8] for s in range(S)])
        d_frames = ctx.alloc(frames.nbytes)
        d_frames.upload(frames)
        views = [DeviceImage(d_frames.ptr.value + s * rows * cols, rows, cols) for s in range(S)]
        batches = {}
        for name, st in (("device", on_settings), ("host", on_settings), ("off", settings)):
            b = MapBatch(ctx, S, K, **st)
            b.configure()
            batches[name] = b
        sessions = list(range(S))
        kw = {"device": dict(images=views), "host": dict(images=frames), "off": {}}
        t_feed = {name: [] for name in batches}
        names = list(batches)
        for k in range(K):
            args = (sessions, [k] * S, [Pose2(poses[k][0] + s, poses[k][1], poses[k][2]) for s in sessions], ping, [clouds[k]] * S)
            for name in names[k % 3:] + names[:k % 3]:
                t = timed(lambda: (batches[name].add_keyframes(*args, **kw[name]), ctx.sync()))
                if k:               # step 0: geometry upload, first allocations
                    t_feed[name].append(t)
        same = all(np.array_equal(batches["device"].maps[s].intensity_grid, batches["host"].maps[s].intensity_grid)
                   for s in (0, S - 1))
        out["lockstep_feed"] = {"sessions": S, "steps": K, "ping_bytes_per_step": int(frames.nbytes),
                                "add_keyframes_ms": {name: med(v) for name, v in t_feed.items()},
                                "add_keyframes_ms_min": {name: float(np.min(v)) for name, v in t_feed.items()},
                                "apply_rounds": {name: b.last_apply_rounds for name, b in batches.items()},
                                "grids_equal": bool(same)}
        for b in batches.values():
            b.close()
        d_frames.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=1000)
    ap.add_argument("--ref-adds", type=int, default=20)
    ap.add_argument("--sessions", type=int, default=None, help="default 32; with --feed store, 0 or absent: a single Mapping")
    ap.add_argument("--batch-keyframes", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--feed", choices=("host", "store"), default=None)
    ap.add_argument("--method", type=int, choices=(1, 2), default=1, help="2: time get_occupancy_grid2 only")
    ap.add_argument("--intensity", action="store_true", help="time the intensity mosaic only")
    a = ap.parse_args()
    n = a.keyframes
    ping = mapping_ref.SessionPing(512, 1024, 30.0 / 1024)
    settings = dict(x0=-100.0, y0=-100.0, width=200.0, height=200.0)
    if a.intensity:
        ctx = _lib.default_context()
        print(json.dumps({"tool": "mapping_times", "device": ctx.name(),
                          "intensity": intensity(ctx, ping, settings, a.keyframes, a.ref_adds, a.sessions or 0,
                                                 a.batch_keyframes, a.reps)}))
        return
    if a.method == 2 and a.feed is not None:
        ctx = _lib.default_context()
        routes = ("host", "store") if a.feed == "store" else ("host",)
        print(json.dumps({"tool": "mapping_times", "device": ctx.name(),
                          "method2_store": method2_store(ctx, ping, settings, a.sessions or 0, a.batch_keyframes, a.reps, routes)}))
        return
    if a.method == 2:
        ctx = _lib.default_context()
        print(json.dumps({"tool": "mapping_times", "device": ctx.name(),
                          "method2": method2(ctx, ping, settings, a.sessions or 0, a.batch_keyframes, a.reps)}))
        return
    if a.feed == "store" and not a.sessions:
        ctx = _lib.default_context()
        print(json.dumps({"tool": "mapping_times", "device": ctx.name(),
                          "feed_single": feed_single(ctx, ping, settings, a.batch_keyframes)}))
        return
    if a.sessions is None:
        a.sessions = 32
    if a.feed is not None:
        ctx = _lib.default_context()
        print(json.dumps({"tool": "mapping_times", "device": ctx.name(),
                          "feed": feed(ctx, ping, settings, max(a.sessions, 1), a.batch_keyframes, a.feed)}))
        return
    poses, clouds = session(n)
    ctx = _lib.default_context()

    dev = Mapping(ctx)
    ref = mapping_ref.Mapping()
    ref.remove_outlier = oracle.remove_outlier
    for m in (dev, ref):
        for k, v in settings.items():
            setattr(m, k, v)
        m.configure()

    dev.add_keyframe(0, Pose2(*poses[0]), ping, clouds[0])     # warm-up: geometry upload, first allocations
    ctx.sync()
    t_dev = []
    for k in range(1, n):
        t_dev.append(timed(lambda: (dev.add_keyframe(k, Pose2(*poses[k]), ping, clouds[k]), ctx.sync())))
    t_ref = []
    for k in range(n):
        if k < a.ref_adds:
            t_ref.append(timed(lambda: ref.add_keyframe(k, Pose2(*poses[k]), ping, clouds[k])))
        else:
            ref.add_keyframe_logodds(k, Pose2(*poses[k]), ping, dev.keyframes[k].logodds)

    out = {"tool": "mapping_times", "device": ctx.name(), "keyframes": n, "image": list(dev.oculus_image_size),
           "add_keyframe_ms": {"device": float(np.median(t_dev)), "numpy": float(np.median(t_ref))},
           "update_poses_ms": {}}
    shift = 0.0
    for K in (100, 1000):
        K = min(K, n)
        shift += 0.7
        new = [Pose2(poses[k][0] + shift, poses[k][1] - shift, poses[k][2] + 0.01 * shift) for k in range(K)]
        td = timed(lambda: (dev.update_poses(list(range(K)), new), ctx.sync()))

        def ref_loop():
            for k in range(K):
                ref.update_pose(k, new[k])
        tr = timed(ref_loop)
        out["update_poses_ms"][str(K)] = {"device": td, "numpy": tr}
    dev.get_occupancy_grid1()
    rd = [timed(dev.get_occupancy_grid1) for _ in range(3)]
    rr = [timed(ref.get_occupancy_grid1) for _ in range(3)]
    out["render_ms"] = {"device": float(np.median(rd)), "numpy": float(np.median(rr)),
                        "box": [int(ref.rmax - ref.rmin + 1), int(ref.cmax - ref.cmin + 1)]}
    out["grid_rows_cols"] = [int(dev.rows), int(dev.cols)]
    out["box_equal"] = [dev.rmin, dev.rmax, dev.cmin, dev.cmax] == [ref.rmin, ref.rmax, ref.cmin, ref.cmax]
    if a.sessions > 0:
        out["lockstep"] = lockstep(ctx, ping, settings, a.sessions, a.batch_keyframes, a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
