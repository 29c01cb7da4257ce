"""Wall time of one SLAM step on N x 3 clouds over store handles (``store.CloudStore3``) next to the same step through the
host-pointer ``pcl`` calls.  A step, for every session: a target from three keyframe clouds (transform, concatenate,
downsample), a scan match of a fourth cloud against it, and the overlap of the matched cloud with the target.

  store route   get_points (all sessions in one call) -> icp (one launch) -> overlap (one launch) -> truncate; the keyframe
                clouds were put once, outside the timed window: that is the point of a store
  host route    per session numpy ``points.dot(H[:3, :3].T) + H[:3, 3]``, np.concatenate and pcl.downsample; one
                pcl.ICP.compute_jobs over all sessions; per session the numpy transform and pcl.match

Both routes run in one process and alternate, call by call; every call ends in a stream synchronisation, so the host clock
around it covers the device work.  Medians and the spread (min .. max) over --reps steps after one warm-up step of each
route.  The results of the two routes are compared bit for bit once per shape.

    python tools/store3_times.py [--shapes 32x800 256x5000] [--reps 5]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sonar_slam_amd import _lib, icp_config, pcl  # noqa: E402
from sonar_slam_amd.store import CloudStore3  # noqa: E402

f32 = np.float32
RESOLUTION, OVERLAP_DIST = 0.1, 0.2


def rigid(axis, angle, t):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    T[:3, 3] = t
    return T


def move(points, H):
    H = np.asarray(H, f32)
    return points.dot(H[:3, :3].T) + H[:3, 3]


def session(seed, n):
    """four keyframes of n points of one world (a 6 x 6 x 4 m box), each in its own frame
    -> (clouds, transforms of the first three into the third's frame, guess for the fourth)"""
    rng = np.random.default_rng(seed)
    world = rng.uniform(-1, 1, (3 * n, 3)) * np.array([3.0, 3.0, 2.0])
    poses = [rigid((0.1, 0.2, 1.0), 0.03 * k, (0.12 * k, -0.05 * k, 0.02 * k)) for k in range(4)]
    clouds = []
    for P in poses:
        seen = world[rng.permutation(len(world))[:n]] + rng.normal(0, 0.004, (n, 3))
        Pi = np.linalg.inv(P)
        clouds.append((seen @ Pi[:3, :3].T + Pi[:3, 3]).astype(f32))
    ref = np.linalg.inv(poses[2])
    between = [np.asarray(ref @ poses[i], f32) for i in range(3)]
    guess = np.asarray(ref @ poses[3] @ rigid((0, 0, 1), 0.01, (0.02, -0.01, 0.01)), f32)
    return clouds, between, guess


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["32x800", "256x5000"], help="sessions x points per keyframe cloud")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    ctx = _lib.default_context()
    params = icp_config.shipped_params()
    icp = pcl.ICP(ctx=ctx)
    icp.setParams(params)
    print("store3_times on %s: one step = target from 3 keyframe clouds (resolution %g) + scan match + overlap (%g m); "
          "%d timed steps per route, alternated" % (ctx.name(), RESOLUTION, OVERLAP_DIST, a.reps))
    for shape in a.shapes:
        S, n = (int(v) for v in shape.split("x"))
        data = [session(1000 * S + k, n) for k in range(S)]
        store = CloudStore3(ctx, capacity_points=S * 7 * n + 1024, max_clouds=S * 5 + 8)
        hk = [[store.put(c) for c in clouds] for clouds, _, _ in data]
        ctx.sync()
        base = len(store)
        guesses = [g for _, _, g in data]

        def store_step():
            t = [time.perf_counter()]
            tgt = store.get_points([h[:3] for h in hk], [b for _, b, _ in data], RESOLUTION)
            t.append(time.perf_counter())
            pairs = [[h[3], int(x)] for h, x in zip(hk, tgt)]
            st, T, it = store.icp(pairs, guesses, params)
            t.append(time.perf_counter())
            ov = store.overlap(pairs, list(T), OVERLAP_DIST)
            t.append(time.perf_counter())
            sizes = store.counts(tgt)
            store.truncate(base)
            return np.diff(t), (st, T, it, ov, sizes)

        def host_step():
            t = [time.perf_counter()]
            targets = [pcl.downsample(np.concatenate([move(c, H) for c, H in zip(clouds[:3], between)]), RESOLUTION, ctx=ctx)
                       for clouds, between, _ in data]
            t.append(time.perf_counter())
            srcs = [clouds[3] for clouds, _, _ in data]
            so = np.r_[0, np.cumsum([len(x) for x in srcs])]
            to = np.r_[0, np.cumsum([len(x) for x in targets])]
            jobs4 = np.array([[so[k], len(srcs[k]), to[k], len(targets[k])] for k in range(S)], np.int32)
            st, T, it = icp.compute_jobs(np.concatenate(srcs), np.concatenate(targets), jobs4,
                                         np.stack(guesses).reshape(S, 16))
            t.append(time.perf_counter())
            ov = np.array([int((pcl.match(tg, move(s, H), 1, OVERLAP_DIST, ctx=ctx)[0][0] != -1).sum())
                           for tg, s, H in zip(targets, srcs, T)], np.int32)
            t.append(time.perf_counter())
            return np.diff(t), (st, T, it, ov, np.array([len(x) for x in targets], np.int32))

        _, rs = store_step()
        _, rh = host_step()
        same = all(np.array_equal(x, y, equal_nan=True) for x, y in zip(rs, rh))
        ts, th = [], []
        for _ in range(a.reps):
            ts.append(store_step()[0])
            th.append(host_step()[0])
        ts, th = 1e3 * np.array(ts), 1e3 * np.array(th)
        print("\n%d sessions x %d points per keyframe: targets of %d .. %d points, statuses %s, results of the two routes %s"
              % (S, n, rs[4].min(), rs[4].max(), sorted(set(rs[0].tolist())), "equal bit for bit" if same else "DIFFER"))
        print("  %-14s %28s %28s %8s" % ("ms per step", "store handles", "host pointers", "ratio"))
        for k, name in enumerate(("get_points", "scan match", "overlap")):
            ms, mh = np.median(ts[:, k]), np.median(th[:, k])
            print("  %-14s %9.3f (%8.3f .. %8.3f) %9.3f (%8.3f .. %8.3f) %7.2fx"
                  % (name, ms, ts[:, k].min(), ts[:, k].max(), mh, th[:, k].min(), th[:, k].max(), mh / ms))
        ss, sh = ts.sum(axis=1), th.sum(axis=1)
        print("  %-14s %9.3f (%8.3f .. %8.3f) %9.3f (%8.3f .. %8.3f) %7.2fx"
              % ("step", np.median(ss), ss.min(), ss.max(), np.median(sh), sh.min(), sh.max(), np.median(sh) / np.median(ss)))
        store.close()
        if not same:
            sys.exit("the two routes differ")


if __name__ == "__main__":
    main()
