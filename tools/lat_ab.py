#!/usr/bin/env python
"""Single scan match latency (host wall clock per pcl.ICP.compute call, shipped chain) of the sweep kernels vs the
brute-force kernel (sfe_icp_set_tuning bit 2) on small clouds, and the GPU time of a resident batch of such jobs.

    python tools/lat_ab.py [--single] [--chain] [--calls 30]

--single leaves the resident batch out; --chain times the single call with a reading MaxDist stage and MedianDist in
the chain (the filter pass and the *_chain_ext entry point) instead of the shipped one."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sonar_slam_amd import _lib, icp_config, pcl, synth  # noqa: E402
from sonar_slam_amd.pipeline import ScanMatchBatch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_legs import timed  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--single", action="store_true")
ap.add_argument("--chain", action="store_true")
ap.add_argument("--calls", type=int, default=30)
a = ap.parse_args()
ctx = _lib.default_context()
icp = pcl.ICP(ctx)
icp.setParams(icp_config.shipped_params())
if a.chain:
    icp.setChain(icp_config.parse_icp_chain(
        "readingDataPointsFilters:\n  - MaxDistDataPointsFilter: {dim: -1, maxDist: 40.0}\n"
        "outlierFilters:\n  - MaxDistOutlierFilter: {maxDist: 3.0}\n  - TrimmedDistOutlierFilter: {ratio: 0.8}\n"
        "  - MedianDistOutlierFilter: {factor: 3.0}\n"
        "transformationCheckers:\n  - CounterTransformationChecker: {maxIterationCount: 40}\n"
        "  - DifferentialTransformationChecker: {minDiffRotErr: 0.01, minDiffTransErr: 0.1, smoothLength: 4}\n"))
for n in (100, 200, 400, 1000):
    s, t, g, _ = synth.scan_pair(seed=40 + n, n_src=n, n_tgt=n)
    for variant in (0, 4):
        ctx._check(ctx.lib.sfe_icp_set_tuning(ctx.handle, variant))
        icp.compute(s, t, g)
        ts = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            icp.compute(s, t, g)
            ts.append(time.perf_counter() - t0)
        if a.single:
            print("%5d points  %-12s single call %7.1f us" % (n, "brute force" if variant else "sweep", 1e6 * np.median(ts)),
                  flush=True)
            continue
        pairs = [synth.scan_pair(seed=9000 + i, n_src=n, n_tgt=n) for i in range(256)]
        nj = 4096
        b = ScanMatchBatch(ctx, icp.params, [pairs[j % 256][0] for j in range(nj)], [pairs[j % 256][1] for j in range(nj)],
                           [(j, j) for j in range(nj)], [pairs[j % 256][2] for j in range(nj)])
        ms = timed(ctx, b.run, 3)
        b.free()
        print("%5d points  %-12s single call %7.1f us   batch of %d: %7.3f ms (%.0f jobs/s)"
              % (n, "brute force" if variant else "sweep", 1e6 * np.median(ts), nj, ms, nj / ms * 1e3), flush=True)
ctx._check(ctx.lib.sfe_icp_set_tuning(ctx.handle, 0))
