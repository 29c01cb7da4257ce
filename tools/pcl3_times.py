"""Wall time of the pcl cloud functions on N x 3 clouds next to the same calls on the (x, y) columns: host arrays in, host
arrays out, so copies and launch latencies are included.  Medians over --reps calls after two warm-up calls; one JSON line.

    python tools/pcl3_times.py [--n 1000 10000] [--reps 9]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sonar_slam_amd import _lib, pcl  # noqa: E402


def med_ms(f, reps):
    for _ in range(2):
        f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return round(1e3 * float(np.median(t)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1000, 10000])
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    ctx = _lib.default_context()
    out = {"tool": "pcl3_times", "device": ctx.name(), "reps": a.reps, "ms": {}}
    for n in a.n:
        rng = np.random.default_rng(n)
        side = float(n) ** (1.0 / 3.0)                      # about one point per unit volume
        p3 = rng.uniform(0, side, (n, 3)).astype(np.float32)
        q3 = rng.uniform(0, side, (max(n // 8, 1), 3)).astype(np.float32)
        row = {}
        for name, p, q in (("3d", p3, q3), ("2d", p3[:, :2].copy(), q3[:, :2].copy())):
            row[name] = {
                "match_knn1": med_ms(lambda: pcl.match(p, q, 1, 1.0, ctx=ctx), a.reps),
                "match_knn3": med_ms(lambda: pcl.match(p, q, 3, 1.0, ctx=ctx), a.reps),
                "remove_outlier": med_ms(lambda: pcl.remove_outlier(p, 1.0, 3, ctx=ctx), a.reps),
                "knn_density5": med_ms(lambda: pcl.knn_density(p, 5, ctx=ctx), a.reps),
                "downsample": med_ms(lambda: pcl.downsample(p, 1.5, ctx=ctx), a.reps),
                "downsample_desc": med_ms(lambda: pcl.downsample(p, p, 1.5, ctx=ctx), a.reps),
            }
        out["ms"][str(n)] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
