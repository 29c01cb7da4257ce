"""Times of ICP with the in-loop outlier filters / checker of ``sfe_icp_outliers`` on the bench shape: 4096 pairs of
5000 x 5000 points, four chains -- the shipped chain; MedianDist{3} in place of TrimmedDist; MinDist + Trimmed; the
shipped chain + Bound (limits never reached).  Each chain runs through ``ICP.compute_jobs`` (one launch, host in / out);
the chains alternate, the best of --reps rounds is kept.  Prints one JSON line.

    python tools/outlier_times.py [--jobs 4096] [--points 5000] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sonar_slam_amd import _lib as L  # noqa: E402
from sonar_slam_amd import icp_config, pcl, synth  # noqa: E402


def chains():
    shipped = icp_config.shipped_params()
    return {
        "shipped": (shipped, None),
        "median3": (icp_config.shipped_params(use_trimmed_filter=0), L.IcpOutliers(use_median=1, median_factor=3.0)),
        "mindist_trimmed": (shipped, L.IcpOutliers(use_min_dist=1, min_dist=0.02)),
        "shipped_bound": (shipped, L.IcpOutliers(use_bound=1, max_rotation_norm=3.0, max_translation_norm=100.0,
                                                 bound_order=1)),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=4096)
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    ctx = L.default_context()
    pairs = [synth.scan_pair(seed=s, n_src=a.points, n_tgt=a.points) for s in range(16)]
    src = np.ascontiguousarray(np.concatenate([q[0] for q in pairs]), np.float32)
    tgt = np.ascontiguousarray(np.concatenate([q[1] for q in pairs]), np.float32)
    j4 = np.array([((j % 16) * a.points, a.points, (j % 16) * a.points, a.points) for j in range(a.jobs)], np.int32)
    g9 = np.stack([pairs[j % 16][2].reshape(9) for j in range(a.jobs)]).astype(np.float32)
    icps = {}
    for name, (p, ox) in chains().items():
        icps[name] = pcl.ICP(ctx)
        icps[name].setChain(icp_config.IcpChain(p, outliers=ox))
    best, res = {}, {}
    for _ in range(a.reps + 1):          # (the first round warms up)
        for name, icp in icps.items():
            t0 = time.perf_counter()
            st, T, it = icp.compute_jobs(src, tgt, j4, g9)
            dt = (time.perf_counter() - t0) * 1e3
            if name in res:
                best[name] = min(best.get(name, dt), dt)
            res[name] = (st.copy(), it.copy())
    out = {"jobs": a.jobs, "points": a.points}
    for name in icps:
        st, it = res[name]
        out[name + "_ms"] = round(best[name], 2)
        out[name + "_mean_iters"] = round(float(it.mean()), 2)
        out[name + "_success"] = int((st == 0).sum())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
