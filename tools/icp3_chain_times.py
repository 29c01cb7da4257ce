"""Wall time of a 3-D ICP chain with a reference octree stage and a MedianDist outlier filter (``icp_config.IcpChain`` with
``dims = 3``: sfe_icp3_dpf.hip and the EXT build of the 3-D job kernel) against the routes that filter on the host side:
``pcl.downsample`` per distinct target cloud through host pointers, then ``pcl.ICP`` on the filtered clouds.  Host arrays in,
host arrays out, at the shapes of tools/icp3_times.py: a single ``compute`` and a ``compute_batch`` of 30 guesses on an
800 x 800 pair, and ``compute_pairs`` on 256 pairs of 5000 x 5000.

    python tools/icp3_chain_times.py [--reps 9] [--pairs 256] [--n 5000] [--resolution 1.0] [--factor 3.0]

Three routes, alternated call by call in one process (two warm-up rounds, then every repeat is printed in ``series``):
  device        the chain with the octree stage on the reference and MedianDist, one call
  host_median   pcl.downsample per target cloud, then the same chain without the stage (MedianDist on the device)
  host_shipped  pcl.downsample per target cloud, then the shipped chain (no MedianDist: all that N x 3 clouds could run before
                chains were taken in 3-D)
``device`` and ``host_median`` compute the same poses bit for bit, which the tool checks.  One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sonar_slam_amd import _lib, icp_config, pcl  # noqa: E402

from icp3_times import pair, rigid  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--resolution", type=float, default=1.0)
    ap.add_argument("--factor", type=float, default=3.0)
    a = ap.parse_args()
    ctx = _lib.default_context()
    rng = np.random.default_rng(1)
    truth = rigid((0, 0, 1), 0.087, (0.8, -0.3, 0.0))
    guess = np.asarray(rigid((0, 0, 1), 0.052, (0.3, -0.2, 0.0)) @ truth, np.float32)
    s, t = pair(rng, 800, truth)
    guesses = [np.asarray(rigid((0, 0, 1), rng.uniform(-0.05, 0.05), np.r_[rng.uniform(-0.3, 0.3, 2), 0]) @ truth, np.float32)
               for _ in range(30)]
    big = [pair(rng, a.n, truth) for _ in range(a.pairs)]
    srcs, tgts, gb = [p[0] for p in big], [p[1] for p in big], [guess] * len(big)

    stage = _lib.IcpDpf(kind=_lib.DPF_OCTREE_GRID, dim=-1, remove_inside=0)
    stage.f[0] = a.resolution
    median = _lib.IcpOutliers(use_median=1, median_factor=a.factor)
    p = icp_config.shipped_params()
    icps = {"device": pcl.ICP(ctx), "host_median": pcl.ICP(ctx), "host_shipped": pcl.ICP(ctx)}
    icps["device"].setChain(icp_config.IcpChain(p, reference=[stage], outliers=median, dims=3))
    icps["host_median"].setChain(icp_config.IcpChain(p, outliers=median, dims=3))
    icps["host_shipped"].setParams(p)

    def ds(c):
        return pcl.downsample(c, a.resolution, ctx=ctx)

    def route(name, shape):
        icp = icps[name]
        if name == "device":
            return {"compute": lambda: icp.compute_batch(s, t, [guess]), "batch": lambda: icp.compute_batch(s, t, guesses),
                    "pairs": lambda: icp.compute_pairs(srcs, tgts, gb)}[shape]
        return {"compute": lambda: icp.compute_batch(s, ds(t), [guess]), "batch": lambda: icp.compute_batch(s, ds(t), guesses),
                "pairs": lambda: icp.compute_pairs(srcs, [ds(c) for c in tgts], gb)}[shape]

    names = {"compute": "compute_800x800", "batch": "compute_batch_30_guesses_800x800",
             "pairs": "compute_pairs_%d_x_%dx%d" % (a.pairs, a.n, a.n)}
    out = {"tool": "icp3_chain_times", "device": ctx.name(), "reps": a.reps, "resolution": a.resolution, "factor": a.factor,
           "series": {k: {} for k in icps}, "ms": {k: {} for k in icps}, "kept_target_points": {}, "iterations": {},
           "device_over_host_median": {}, "device_over_host_shipped": {}}
    for shape, reps in (("compute", a.reps), ("batch", a.reps), ("pairs", max(a.reps // 3, 3))):
        ser = {k: [] for k in icps}
        last = {}
        for r in range(reps + 2):                      # two warm-up rounds, then alternate call by call
            for k in icps:
                t0 = time.perf_counter()
                last[k] = route(k, shape)()
                if r >= 2:
                    ser[k].append(round(1e3 * (time.perf_counter() - t0), 4))
        same = all(np.array_equal(x, y) for x, y in zip(last["device"][1:], last["host_median"][1:]))
        if not same or list(last["device"][0]) != list(last["host_median"][0]):
            raise SystemExit("icp3_chain_times: the device route and the host route differ at %s" % names[shape])
        for k in icps:
            out["series"][k][names[shape]] = ser[k]
            out["ms"][k][names[shape]] = round(float(np.median(ser[k])), 4)
        out["iterations"][names[shape]] = {k: round(float(np.mean(last[k][2])), 2) for k in icps}
        out["device_over_host_median"][names[shape]] = round(out["ms"]["device"][names[shape]] / out["ms"]["host_median"][names[shape]], 3)
        out["device_over_host_shipped"][names[shape]] = round(out["ms"]["device"][names[shape]] / out["ms"]["host_shipped"][names[shape]], 3)
    out["kept_target_points"] = {"800": int(len(ds(t))), str(a.n): round(float(np.mean([len(ds(c)) for c in tgts[:8]])), 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
