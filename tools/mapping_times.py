"""Times of the device occupancy map (sonar_slam_amd.mapping) next to the numpy restatement of the reference
(tests/mapping_ref.py) on the same synthetic session: 1024 ranges x 512 beams at 30 m, the shipped 0.2 m map resolution.
Prints one JSON line:
  add_keyframe_ms        per add_keyframe from points (outlier filter, measurement, fit, add)
  update_poses_ms        update_poses with K = 100 and K = 1000 keyframes all changed (device: one call; numpy: the
                         update_pose loop of the reference)
  render_ms              get_occupancy_grid1() over the whole box (about 1000 x 1000 cells)
The numpy side adds only `--ref-adds` keyframes from points (the rest through add_keyframe_logodds, which skips the
measurement) to keep the run short.

    python tools/mapping_times.py [--keyframes 1000] [--ref-adds 20]
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
import mapping_ref  # noqa: E402
import oracle  # noqa: E402
from sonar_slam_amd import _lib  # noqa: E402
from sonar_slam_amd.mapping import Mapping  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=1000)
    ap.add_argument("--ref-adds", type=int, default=20)
    a = ap.parse_args()
    n = a.keyframes
    ping = mapping_ref.SessionPing(512, 1024, 30.0 / 1024)
    settings = dict(x0=-100.0, y0=-100.0, width=200.0, height=200.0)
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
    print(json.dumps(out))


if __name__ == "__main__":
    main()
