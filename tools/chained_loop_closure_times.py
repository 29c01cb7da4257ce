#!/usr/bin/env python
"""Wall time of the loop-closure search in lock-step: chained.SessionBatch(nssm_enable=True) over S closed-loop sessions
(13 keyframes per lap, the search on from keyframe 8), against the same sessions through S sequential
replay.FrontEnd(store=..., nssm_enable=True) runs.

Per S it prints one JSON line: the batch's per-step wall time (mean over the steps that search), split into the search's device
stages (the store calls, the cost grids and the cost launch, the ICPs and overlaps: host time spent inside them, synchronisations
included), its host shgo replays / scipy fallbacks, its MinCovDet, and the rest of the step (feature extraction, sequential scan
match with its global initialisation); then the sequential FrontEnd runs' total and the ratio.  The records of both are compared
session by session (the search records bit for bit), so a timing never comes from a run that computed something else.

    python tools/chained_loop_closure_times.py [--sessions 1 8 32] [--keyframes 20] [--rows 256] [--beams 128]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sonar_slam_amd import _lib, chained, icp_config, synth  # noqa: E402
from sonar_slam_amd import store as st  # noqa: E402
from sonar_slam_amd.CFAR import CFAR  # noqa: E402
from sonar_slam_amd.feature_extraction import FeatureExtraction, SonarPing, oculus_bearings  # noqa: E402
from sonar_slam_amd.replay import FrontEnd, replay  # noqa: E402

SETTINGS = dict(nssm_min_points=30, mcd_random_state=0)


def sessions(S, K, rows, beams, world):
    bearings = oculus_bearings(beams)
    pings, drs = [], []
    for s in range(S):
        true, dr = synth.trajectory(n=K, step=1.7, turn=2 * np.pi / 13, seed=21 + 4 * s,
                                    start=(20.0 - 1.5 * (s % 8), 0.8 * (s % 5), 0.1 * (s % 3)))
        pings.append(np.array([synth.render_ping(world, true[k], bearings, rows=rows, seed=100 * s + k) for k in range(K)]))
        drs.append(dr)
    return np.array(pings), np.array(drs), bearings


def feature_extraction(ctx, ping):
    fe = FeatureExtraction(ctx)
    fe.Ntc, fe.Ngc, fe.Pfa, fe.rank, fe.alg, fe.threshold = 40, 10, 0.1, 10, "SOCA", 65
    fe.resolution, fe.outlier_filter_radius, fe.outlier_filter_min_points, fe.skip = 0.5, 1.0, 5, 1
    fe.configure()
    fe.generate_map_xy(ping)
    return fe


def batch_run(ctx, det, pings, dr, bearings, rows):
    S, K = pings.shape[:2]
    fe = feature_extraction(ctx, SonarPing(pings[0, 0], bearings, 30.0 / rows))
    sb = chained.SessionBatch(ctx, fe.geometry, det.params["SOCA"], "SOCA", 65, icp_config.shipped_params(), S, K, dr,
                              ssm_min_points=20, initialization=True, nssm_enable=True, **SETTINGS)
    for k in range(K):
        sb.upload_frames(k, pings[:, k])
    sb.warm_up()
    sb.run()                                    # (untimed: scratch growth, first launches)
    sb.reset()
    base = dict(sb.nssm_stats)
    steps = []
    for k in range(K):
        t0 = time.perf_counter()
        sb.step(k)
        steps.append(time.perf_counter() - t0)
    stats = {key: sb.nssm_stats[key] - base[key] for key in base}
    recs, loops = sb.records, sb.loops
    sb.free()
    return np.array(steps), stats, recs, loops


def front_end_runs(ctx, pings, dr, bearings, rows):
    S, K = pings.shape[:2]
    logs, t = [], 0.0
    fe = feature_extraction(ctx, SonarPing(pings[0, 0], bearings, 30.0 / rows))
    for s in range(S):
        store = st.CloudStore(ctx, capacity_points=1 << 19, max_clouds=512)
        # (every ping a keyframe, as in the batch: a short odometry step must not make FrontEnd skip one)
        front = FrontEnd(ctx, keyframe_translation=0.0, keyframe_duration=0.5, store=store, ssm_min_points=20, nssm_enable=True,
                         **SETTINGS)
        front.warm_up()
        sp = [SonarPing(p, bearings, 30.0 / rows, ping_id=k) for k, p in enumerate(pings[s])]
        t0 = time.perf_counter()
        log, _, _ = replay(sp, np.arange(K, dtype=float), dr[s], fe, front)
        t += time.perf_counter() - t0
        logs.append((log, [f for f in front.backend.factors if f[0] == "loop"]))
        store.close()
    return t, logs


def same(recs, loops, logs):
    """-> True, or where the batch's records first differ from FrontEnd's"""
    for s, (log, lf) in enumerate(logs):
        if len(log) != len(recs) or len(lf) != len(loops[s]):
            return "session %d: %d / %d keyframes, %d / %d loops" % (s, len(recs), len(log), len(loops[s]), len(lf))
        for k, (r, a) in enumerate(zip(recs, log)):
            nb, na = r["nssm"][s], a.get("nssm")
            if chained.STATUS_NAMES[r["status"][s]] != a["status"] or tuple(r["pose"][s]) != a["pose"]:
                return "session %d step %d: scan match %s / %s" % (s, k, chained.STATUS_NAMES[r["status"][s]], a["status"])
            if (nb is None) != (na is None) or (nb is not None and set(nb) != set(na)):
                return "session %d step %d: search record keys %s / %s" % (s, k, nb and sorted(nb), na and sorted(na))
            for key in nb or ():
                if not np.array_equal(np.asarray(nb[key]), np.asarray(na[key])):
                    return "session %d step %d: search %s %s / %s" % (s, k, key, nb[key], na[key])
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--keyframes", type=int, default=20)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--beams", type=int, default=128)
    a = ap.parse_args()
    ctx = _lib.default_context()
    det = CFAR(40, 10, 0.1, 10)
    world = synth.world_structure(seed=2, n=9000)
    for S in a.sessions:
        pings, dr, bearings = sessions(S, a.keyframes, a.rows, a.beams, world)
        steps, stats, recs, loops = batch_run(ctx, det, pings, dr, bearings, a.rows)
        t_fe, logs = front_end_runs(ctx, pings, dr, bearings, a.rows)
        searching = [k for k, r in enumerate(recs) if any(x is not None for x in r.get("nssm", []))]
        n_step = max(len(searching), 1)
        statuses = {}
        for r in recs:
            for x in r["nssm"]:
                if x is not None:
                    statuses[x["status"]] = statuses.get(x["status"], 0) + 1
        out = {
            "sessions": S, "keyframes": a.keyframes, "rows": a.rows, "beams": a.beams, "searching_steps": len(searching),
            "searches": stats["searches"], "search_statuses": statuses, "loops": sum(len(x) for x in loops),
            "batch_total_s": round(float(steps.sum()), 4),
            "batch_step_ms_searching": round(1e3 * float(steps[searching].mean()), 2) if searching else None,
            "search_ms_per_step": {"device_stages": round(1e3 * stats["device_s"] / n_step, 2),
                                   "host_shgo": round(1e3 * stats["shgo_s"] / n_step, 2),
                                   "mincovdet": round(1e3 * stats["mcd_s"] / n_step, 2),
                                   "search_total": round(1e3 * stats["host_s"] / n_step, 2)},
            "search_ms_per_session_search": round(1e3 * stats["host_s"] / max(stats["searches"], 1), 3),
            "front_end_sequential_total_s": round(t_fe, 4),
            "speedup_vs_sequential": round(t_fe / float(steps.sum()), 2),
            "records_equal_front_end": same(recs, loops, logs),
        }
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
