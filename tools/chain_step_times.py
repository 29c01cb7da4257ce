"""Cost of a whole ICP chain on the resident path: ms per ``chained.SessionBatch.step`` with the shipped params against a
chain with data-point filters and an outlier filter (a reading MaxDist, a reference octree, MedianDist), on the same
sessions.  The two alternate run by run (after an untimed warm-up of each); the mean and best of --reps runs per chain
are printed as one JSON line.  The scan matches differ between the chains (the chain changes the poses), so the numbers
include whatever the chain does to the iteration counts.

    python tools/chain_step_times.py [--sessions 32] [--steps 8] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sonar_slam_amd import _lib as L  # noqa: E402
from sonar_slam_amd import chained, icp_config, synth  # noqa: E402
from sonar_slam_amd.CFAR import CFAR  # noqa: E402
from sonar_slam_amd.feature_extraction import FeatureExtraction, SonarPing, oculus_bearings  # noqa: E402

CHAIN = """readingDataPointsFilters:
  - MaxDistDataPointsFilter: {dim: -1, maxDist: 20.0}
referenceDataPointsFilters:
  - OctreeGridDataPointsFilter: {maxSizeByNode: 0.7, samplingMethod: 3}
matcher:
  KDTreeMatcher: {knn: 1, epsilon: 0, maxDist: 10.0}
outlierFilters:
  - MaxDistOutlierFilter: {maxDist: 3.0}
  - TrimmedDistOutlierFilter: {ratio: 0.8}
  - MedianDistOutlierFilter: {factor: 3.0}
errorMinimizer: PointToPointErrorMinimizer
transformationCheckers:
  - CounterTransformationChecker: {maxIterationCount: 40}
  - DifferentialTransformationChecker: {minDiffRotErr: 0.01, minDiffTransErr: 0.1, smoothLength: 4}
inspector: NullInspector
logger: NullLogger
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=32)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    S, K, rows, beams = a.sessions, a.steps, 512, 256
    ctx = L.default_context()
    world = synth.world_structure(seed=2, n=8000)
    bearings = oculus_bearings(beams)
    frames = np.zeros((K, S, rows, beams), np.uint8)
    dr = np.zeros((S, K, 3))
    for s in range(S):
        t, d = synth.trajectory(n=K, step=1.7, turn=0.03 + 0.01 * (s % 4), start=(2.0 + 0.5 * (s % 8), 0.3 * (s % 8) - 1.0,
                                                                                0.02 * s), seed=100 + s)
        dr[s] = d
        for k in range(K):
            frames[k, s] = synth.render_ping(world, t[k], bearings, rows=rows, seed=1000 * s + k)
    fe = FeatureExtraction(ctx)
    fe.Ntc, fe.Ngc, fe.Pfa, fe.rank, fe.alg, fe.threshold = 40, 10, 0.1, 10, "SOCA", 65
    fe.configure()
    fe.generate_map_xy(SonarPing(frames[0, 0], bearings, 30.0 / rows))
    chains = {"shipped": icp_config.shipped_params(), "filters_median": icp_config.parse_icp_chain(CHAIN)}
    sb = chained.SessionBatch(ctx, fe.geometry, CFAR(40, 10, 0.1, 10).params["SOCA"], "SOCA", 65, chains["shipped"], S, K, dr)
    for k in range(K):
        sb.upload_frames(k, frames[k])
    ms = {name: [] for name in chains}
    converged = {}
    for rep in range(a.reps + 1):
        for name in (chains if rep % 2 == 0 else list(chains)[::-1]):
            sb.icp_params = chains[name]
            ctx.sync()
            t0 = time.perf_counter()
            recs = sb.run()
            ctx.sync()
            if rep:                                 # rep 0: warm-up (scratch growth, first launches)
                ms[name].append(1e3 * (time.perf_counter() - t0) / K)
            converged[name] = int(sum((r.get("icp_status", np.full(S, -1)) == 0).sum() for r in recs))
    sb.free()
    print(json.dumps({"sessions": S, "steps": K, "reps": a.reps, "device": ctx.name(),
                      "ms_per_step_mean": {n: round(float(np.mean(v)), 3) for n, v in ms.items()},
                      "ms_per_step_best": {n: round(float(np.min(v)), 3) for n, v in ms.items()},
                      "ms_per_step_runs": {n: [round(x, 3) for x in v] for n, v in ms.items()},
                      "scan_matches_converged": converged}))


if __name__ == "__main__":
    main()
