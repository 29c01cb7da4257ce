#!/usr/bin/env python
"""Sonar front-end throughput on MI355X: keyframes/s for CFAR -> cloud -> ICP.

    python bench.py --gpus 1 --steps 5 --warmup 1
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A "step" = one pass of the hot path over a batch of B synthetic keyframes resident in HBM:
B sonar pings (1024 range bins x 512 beams, uint8) through SOCA-CFAR + intensity gate +
polar->Cartesian point extraction + pcl.downsample + pcl.remove_outlier (= the whole of
FeatureExtraction.callback), and B scan pairs (5000 x 5000 points) through the 30-iteration
2-D point-to-plane ICP (BASELINE.json configs[1]).  Every rank owns one GPU and its own B jobs
(weak scaling, no data-path collective; torch.distributed/gloo is control plane only: barrier
and the max-over-ranks time).  Rank 0 prints ONE JSON line.

A plain run does only what that line's headline figure needs: set-up, warm-up, the timed steps, --dump-outputs if given,
and the line (`value`, `ms_per_step` and `config`).  --full adds everything else the bench measures or checks, as it did
before the option existed: the CPU baseline, the oracle parity sample of the timed batch, per-stage times, rooflines and
the counted ICP utilisation, the legs of tools/bench_legs.py, live latency and the farm leg.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
ROWS, COLS = 1024, 512     # range bins x beams
N_PTS = 5000


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=4096,
                    help="keyframes per step per GPU (512 = one scan match per workgroup slot of the 256 CUs: every job's "
                         "tail is exposed; with several times more the dispatcher refills slots as jobs finish: -15 %% per job at 2048, "
                         "-19 %% at 4096)")
    ap.add_argument("--full", action="store_true",
                    help="measure and check everything beyond the headline figure as well: CPU baseline, parity sample, "
                         "per-stage times and rooflines, legs, live latency, farm (the options below marked --full)")
    ap.add_argument("--cfar-frames", type=int, default=1024, help="frames per launch for the CFAR roofline leg (--full)")
    ap.add_argument("--inflight", type=int, default=1,
                    help="keyframe batches in flight per GPU: consecutive steps alternate between this many resident "
                         "batches, each on its own context (stream + scratch), so the front end and the ICP preparation "
                         "of step k+1 fill the CUs the iteration kernel of step k leaves idle (default 1 = one batch, serial; "
                         "measured on MI355X: 114.6 k keyframes/s with 1, 116.3 k with 2, 118.9 k with 3)")
    ap.add_argument("--cfar-launches", type=int, default=20, help="launches per timing of the CFAR roofline leg (--full)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="skip the CPU baseline (--full)")
    ap.add_argument("--cpu-keyframes", type=int, default=0,
                    help="CPU-baseline keyframes per host core (0 = about 10 s of work per core; --full)")
    ap.add_argument("--icp-mode", choices=["p2plane30", "reference"], default="p2plane30")
    ap.add_argument("--no-filters", action="store_true", help="leave pcl.downsample / remove_outlier out of the step")
    ap.add_argument("--max-points", type=int, default=32768,
                    help="point capacity per frame.  The synthetic frames of some ranks hold pings of > 16384 detections (seed 3002: "
                         "19 122): the 8-rank launch of round 6 found rank 3 raising at the 16384 of rounds 1-5.  The resident "
                         "filters pick their sort per frame, so the capacity only sizes buffers")
    ap.add_argument("--parity-jobs", type=int, default=64,
                    help="keyframes of the timed batch re-computed by the oracle after the timed region (0 = skip; --full)")
    ap.add_argument("--no-farm", action="store_true", help="skip the BASELINE configs[3] leg (job farm on this device; --full)")
    ap.add_argument("--farm-jobs", type=int, default=10000, help="jobs of the farm leg (--full)")
    ap.add_argument("--no-latency", action="store_true",
                    help="skip the live single-ping / single-scan-match latency leg (--full)")
    ap.add_argument("--distinct-frames", type=int, default=256,
                    help="distinct synthetic pings behind the batch's frames (tiled to --batch); beyond the first 32 they are "
                         "screened on the device, untimed: a ping with more points than the batch's capacity is left out")
    ap.add_argument("--no-legs", action="store_true",
                    help="skip the legs beyond the timed step: reference_chain, real_size, configs4_hires, float_oracle, "
                         "stream_frames (--full)")
    ap.add_argument("--small-legs", action="store_true", help="those legs at a fraction of their size (tests; --full)")
    ap.add_argument("--serial-prep", action="store_true",
                    help="keep the ICP target preparation on the main stream (default: side stream, next to the front end)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step computed (rank 0) to DIR/<name>.npy, float32 / float64: the "
                         "per-keyframe ICP results and point counts of the whole batch, and the CFAR masks, points and "
                         "filtered clouds of a fixed sample of its frames (see dump_outputs)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


def make_inputs(rank, batch):
    from sonar_slam_amd import synth
    n_distinct = min(batch, 32)
    base = [synth.sonar_frame(seed=1000 * rank + s) for s in range(n_distinct)]
    frames = np.stack([base[j % n_distinct] for j in range(batch)])
    srcs, tgts, guesses = [], [], []
    for j in range(batch):
        s, t, g, _ = synth.scan_pair(seed=100000 * rank + j, n_src=N_PTS, n_tgt=N_PTS)
        srcs.append(s)
        tgts.append(t)
        guesses.append(g)
    return frames, srcs, tgts, np.stack(guesses)


_CPU = {}


def usable_cores():
    """CPUs this process may really use: affinity mask and cgroup quota, not the host's core count."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        pass
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(int(txt[0]) / int(txt[1]))))
            else:
                q = int(txt[0])
                per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                if q > 0:
                    n = min(n, max(1, q // per))
        except (OSError, ValueError, IndexError):
            pass
    return n


def _cpu_keyframe(j):
    """One keyframe through the oracle: the reference's per-ping + per-scan-match CPU work."""
    import oracle
    c = _CPU
    t0 = time.perf_counter()
    m = oracle.gate(c["frames"][j], oracle.cfar(c["frames"][j], "SOCA", c["th"], c["gh"], c["tau"]), 65)
    t1 = time.perf_counter()
    rc = oracle.nonzero(oracle.remap_u8(m, c["map_x"], c["map_y"]))
    pts = oracle.px_to_m(rc, c["rows"], c["cols"], c["width"], c["height"])
    if c["filters"] and len(pts):
        pts = oracle.downsample(pts.astype(np.float32), 0.5)               # feature_extraction.py:241-249
        if len(pts):
            oracle.remove_outlier(np.asarray(pts, np.float32), 1.0, 5)
    t2 = time.perf_counter()
    oracle.icp(c["srcs"][j], c["tgts"][j], c["guesses"][j], c["prm"])
    return t1 - t0, t2 - t1, time.perf_counter() - t2


def cpu_baseline(frames, srcs, tgts, guesses, n_kf, det, fe, icp_mode, filters=True):
    """The oracle (C port of the reference path, built with the reference's flags: -O3, no -march=native)
    on a bounded sample of the same keyframes, one independent worker process per host core (the
    reference is single-threaded per node process).  NN search = the oracle's exact kd-tree, like
    libpointmatcher's KDTreeMatcher (same neighbours as brute force, tests/test_oracle_pipeline.py)."""
    import multiprocessing as mp

    import oracle
    th, gh, tau = det.params["SOCA"]
    if icp_mode == "p2plane30":
        prm = oracle.shipped_icp_params(minimizer=1, use_diff_checker=0, max_iter=30, precision=0)
    else:
        prm = oracle.shipped_icp_params(precision=0)
    oracle.set_kdtree(1)
    _CPU.update(frames=frames, srcs=srcs, tgts=tgts, guesses=guesses, th=th, gh=gh, tau=tau, map_x=fe.map_x,
                map_y=fe.map_y, rows=fe.rows, cols=fe.cols, width=fe.width, height=fe.height, prm=prm, filters=filters)
    cores = usable_cores()
    nb = len(frames)
    t0 = time.perf_counter()
    one = [_cpu_keyframe(j) for j in range(min(4, nb))]            # 1 core
    dt1 = time.perf_counter() - t0
    # batches of keyframes (the step's own, cycled) until about 10 s have passed, so that the sample is
    # bounded by time whatever the host looks like
    budget_s = 10.0 if not n_kf else 1e9
    done = 0
    try:
        with mp.get_context("fork").Pool(cores) as pool:           # fork: the workers inherit the inputs
            pool.map(_cpu_keyframe, [j % nb for j in range(cores)])  # warm the pool
            t0 = time.perf_counter()
            while True:
                batch = [(done + j) % nb for j in range(2 * cores if not n_kf else n_kf * cores)]
                pool.map(_cpu_keyframe, batch, chunksize=1)
                done += len(batch)
                if n_kf or time.perf_counter() - t0 >= budget_s:
                    break
            dt = time.perf_counter() - t0
    finally:
        oracle.set_kdtree(0)
    n_kf = done
    ref_note = ""
    if oracle.have_ref_cfar():   # the reference's own cfar.cpp (oracle/_ref), incl. pybind's uint8 -> float cast-copy
        t0 = time.perf_counter()
        for j in range(2):
            oracle.ref_cfar(frames[j], "SOCA", th, gh, tau)
        ref_note = "; the reference's own cfar.cpp (compiled unmodified): %.1f ms/frame" % (
            1e3 * (time.perf_counter() - t0) / 2)
    return {"value": n_kf / dt, "unit": "keyframes/s", "cores": cores, "kind": "port",
            "sample": "%d keyframes (1024x512 SOCA-CFAR+gate+remap+nonzero+px2m+downsample+remove_outlier, 5000x5000 ICP %s with an exact "
                      "kd-tree) in %.1f s on %d worker processes; one core alone: %.2f keyframes/s "
                      "(CFAR %.1f ms, remap+nonzero+filters %.1f ms, ICP %.1f ms per keyframe)%s"
                      % (n_kf, icp_mode, dt, cores, len(one) / dt1, 1e3 * np.mean([o[0] for o in one]),
                         1e3 * np.mean([o[1] for o in one]), 1e3 * np.mean([o[2] for o in one]), ref_note)}


VALU_PEAK_TFLOPS = 157.3    # MI355X_MICROARCH.md: fp32 vector peak
LDS_PEAK_GBS = 256 * 256 * 2.4     # 256 B/clk/CU (ds_read_b64, MI355X_MICROARCH.md LDS table) x 256 CUs x 2.4 GHz


def icp_utilisation(ctx, kb, ms_launch, iters_total, n_jobs):
    """Counted work of the ICP loop kernel (one profiled launch of the same batch: candidate distance evaluations of the
    lane-per-query tiers, the cooperative tier and the witnesses, lower-bound probes) against the fp32 vector peak and the
    LDS peak, next to what an exhaustive search of the same jobs would have evaluated."""
    import ctypes
    prof = (ctypes.c_longlong * 96)()
    ctx._check(ctx.lib.sfe_icp_get_profile(ctx.handle, 1, prof))
    kb.run_icp()
    ctx.sync()
    ctx._check(ctx.lib.sfe_icp_get_profile(ctx.handle, 0, prof))
    evals = int(prof[80]) + int(prof[81]) + int(prof[82])
    probes = int(prof[83])
    iters_counted = int(prof[84])
    flop = 8.0 * evals                                   # 8 flop per pair evaluation
    sec = ms_launch * 1e-3
    out = {"kernel": "icp_sweep_kernel (+ icp_sweep_prep_kernel)", "bound": "valu/salu issue + lds/barrier latency",
           "ms_per_launch": ms_launch, "jobs_per_launch": n_jobs,
           "pair_evals_per_launch": evals, "lower_bound_probes_per_launch": probes,
           "pair_evals_per_query_and_iteration": evals / max(1.0, float(iters_counted) * N_PTS),
           "valu_frac": flop / sec / 1e12 / VALU_PEAK_TFLOPS,
           "valu_note": "8 flop x counted pair evaluations / launch time / 157.3 TFLOP/s fp32 vector peak: the search "
                        "evaluates ~0.1 % of the n_src x n_tgt pairs, the rest of the kernel is control flow, "
                        "selection and fp64 sums",
           "lds_frac": 8.0 * (evals + probes) / sec / 1e9 / LDS_PEAK_GBS,
           "lds_note": "8 B per candidate / probe read from LDS / launch time / 157 TB/s (256 B/clk/CU x 256 CUs x 2.4 GHz)",
           "exhaustive_pairs_per_launch": float(N_PTS) * N_PTS * iters_total,
           "pruning_factor": float(N_PTS) * N_PTS * iters_total / max(1, evals)}
    if iters_counted != iters_total:
        out["note"] = "profiled launch ran %d iterations, timed launch %d" % (iters_counted, iters_total)
    return out


def farm_leg(icp_p, srcs, tgts, guesses, n_jobs):
    """BASELINE configs[3] at N = 1: n_jobs independent 5000 x 5000 scan matches through farm.IcpFarm (one persistent
    worker process per device -- here this rank's device only --, jobs over shared memory, 1024 per launch), host wall
    clock per batch incl. packing, host<->device copies and unpacking; every job has its own guess."""
    from sonar_slam_amd import synth
    from sonar_slam_amd.farm import IcpFarm
    rng = np.random.default_rng(0)
    nd = min(len(srcs), 512)
    jobs = [(srcs[j % nd], tgts[j % nd], [np.asarray(guesses[j % nd], np.float64)
                                           @ synth.pose_matrix(*rng.normal(0, [0.05, 0.05, 0.005]))])
            for j in range(n_jobs)]
    jobs = [(s, t, [g[0].astype(np.float32)]) for s, t, g in jobs]
    dev = int(os.environ.get("SONARFE_BENCH_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    with IcpFarm(icp_p, devices=[dev]) as farm:
        farm.run(jobs[:64])                                   # worker start-up, scratch growth
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            out = farm.run(jobs)
            times.append(time.perf_counter() - t0)
    ok = sum(m[0] == "success" for m, _, _ in out)
    return {"jobs": n_jobs, "distinct_pairs": nd, "devices": 1, "seconds_per_batch": min(times),
            "jobs_per_s": n_jobs / min(times), "converged": ok,
            "note": "farm.IcpFarm on this device: persistent worker, shared-memory job blocks; 8-GPU scaling = one such "
                    "worker per device, job j -> device j mod G, no collective (not measurable on a 1-GPU box)"}


def pose_diff(Ta, Tb):
    """max(|dx|, |dy|, |dtheta|) between two 3x3 Pose2 matrices: the north_star bar is 1e-4 m / 1e-4 rad"""
    dth = np.arctan2(Ta[1, 0], Ta[0, 0]) - np.arctan2(Tb[1, 0], Tb[0, 0])
    return float(max(abs(Ta[0, 2] - Tb[0, 2]), abs(Ta[1, 2] - Tb[1, 2]), abs(np.arctan2(np.sin(dth), np.cos(dth)))))


def parity_check(kb, res, frames, srcs, tgts, guesses, det, fe, icp_mode, filters, k_jobs):
    """Oracle sample of the TIMED batch (the outputs left in HBM by the last timed step): k_jobs keyframes spread
    over the batch, each through the whole oracle chain -- CFAR mask, extracted points (order included), filtered
    cloud: bit-exact; ICP pose: <= 1e-4 m / rad against the oracle in float (PointMatcher<float>) with its exact
    kd-tree, and the same statuses / iteration counts as the oracle with fp64 sums.  Raises on any mismatch: a bench line
    whose work is wrong must not be printed."""
    import oracle
    th, gh, tau = det.params["SOCA"]
    n = len(frames)
    picks = sorted(set(int(round(i * (n - 1) / max(1, k_jobs - 1))) for i in range(k_jobs)))
    mk = dict(minimizer=1, use_diff_checker=0, max_iter=30) if icp_mode == "p2plane30" else {}
    # the batch's outputs come down first (the context is not re-entrant), then the oracle runs the sampled keyframes on
    # the host cores (ctypes releases the GIL; the oracle keeps no shared state besides the kd-tree switch)
    got = {j: (kb.mask(j), kb.points(j), kb.cloud(j) if filters else None) for j in picks}
    oracle.set_kdtree(1)
    try:
        def one(j):
            gm, gp, gc = got[j]
            m = oracle.gate(frames[j], oracle.cfar(frames[j], "SOCA", th, gh, tau), 65)
            if not np.array_equal(gm, m):
                raise AssertionError("parity: CFAR mask of timed frame %d differs from the oracle" % j)
            rc = oracle.nonzero(oracle.remap_u8(m, fe.map_x, fe.map_y))
            pts = oracle.px_to_m(rc, fe.rows, fe.cols, fe.width, fe.height)
            if not np.array_equal(gp, pts):
                raise AssertionError("parity: extracted points of timed frame %d differ from the oracle" % j)
            if filters:
                cl = oracle.remove_outlier(oracle.downsample(pts.astype(np.float32), 0.5), 1.0, 5)
                if not np.array_equal(gc, cl):
                    raise AssertionError("parity: filtered cloud of timed frame %d differs from the oracle" % j)
            st, To, it = oracle.icp(srcs[j], tgts[j], guesses[j], oracle.shipped_icp_params(precision=0, **mk))
            st64, To64, it64 = oracle.icp(srcs[j], tgts[j], guesses[j], oracle.shipped_icp_params(precision=1, **mk))
            if int(res["status"][j]) != st64 or int(res["iters"][j]) != it64:
                raise AssertionError("parity: ICP job %d status/iterations (%d, %d) vs oracle (%d, %d)"
                                     % (j, res["status"][j], res["iters"][j], st64, it64))
            # (third figure: how far the float oracle is from its OWN fp64-sum version on this job -- the bound below)
            return pose_diff(res["T"][j], To), pose_diff(res["T"][j], To64), pose_diff(To, To64)
        from multiprocessing.pool import ThreadPool
        with ThreadPool(max(1, usable_cores())) as tp:
            diffs = tp.map(one, picks, chunksize=1)
    finally:
        oracle.set_kdtree(0)
    bit_exact = len(picks)
    d32 = np.array([d[0] for d in diffs])
    worst64 = float(max(d[1] for d in diffs))
    # the north_star bar (1e-4) against the oracle in float: the jobs beyond it are exactly those where the float oracle
    # leaves its own fp64-sum version by as much (`float_oracle` leg); against the fp64-sum oracle the bar is 1e-6
    beyond = int((d32 > 1e-4).sum())
    worst = float(d32.max())
    if not worst64 <= 1e-6:
        raise AssertionError("parity: ICP pose differs from the oracle (fp64 sums) by %.3e (> 1e-6)" % worst64)
    # Against the float oracle there is no absolute bar to enforce: sequential float sums leave the fp64-sum version of the
    # same chain by 1e-4 .. 6e-3 on 5000-point pairs, job by job (profiles/r05_oracle_soak_seed2828.json).  What must hold
    # is that the HIP pose is no further from the float oracle than the float oracle is from its own fp64-sum version on
    # that job (+ 1e-6, the bar enforced against the fp64-sum version): a difference beyond that is the kernel's.
    self32 = np.array([d[2] for d in diffs])
    excess = float((d32 - self32).max())
    if not excess <= 1e-6:
        j = int(np.argmax(d32 - self32))
        raise AssertionError("parity: ICP job %d is %.3e from the float oracle, which is only %.3e from its own fp64-sum "
                             "version" % (picks[j], d32[j], self32[j]))
    return {"jobs": len(picks), "frames_bit_exact": bit_exact, "icp_max_pose_diff": worst,
            "icp_float_oracle_beyond_1e-4": "%d / %d" % (beyond, len(picks)),
            "icp_max_pose_diff_vs_f64_sums": worst64,
            # what this function ENFORCES (it raises beyond them) and what north_star asks for, kept apart:
            "icp_tolerance_enforced_f64_sums": 1e-6,
            "icp_tolerance_enforced_float_oracle": "per job: <= |float oracle - its own fp64-sum version| + 1e-6",
            "float_oracle_max_distance_from_its_f64_version": float(self32.max()),
            "icp_tolerance_north_star": 1e-4, "north_star_1e-4_met_vs_float_oracle": beyond == 0,
            "north_star_1e-4_met_vs_f64_sum_oracle": worst64 <= 1e-4,
            "icp_tolerance_note": "the float (PointMatcher<float>-style, sequential float sums) oracle leaves its OWN fp64-sum "
                                  "version by up to ~1e-3 on 5000-point pairs; the HIP path equals the fp64-sum version, so "
                                  "jobs beyond 1e-4 of the float oracle are reported, not hidden (DESIGN 3, `float_oracle` leg)",
            "checked": "CFAR mask, extracted points (np.nonzero order), %sICP pose/status/iterations of keyframes %s of "
                       "the last timed step vs the CPU oracle (exact kd-tree)"
                       % ("downsample+remove_outlier cloud, " if filters else "", picks)}


DUMP_FRAMES = 8            # frames of the batch whose per-pixel / per-point outputs are dumped
DUMP_MAX_BYTES = 64 << 20


def dump_outputs(path, kb, res, filters):
    """The outputs of the last timed step, as a caller of KeyframeBatch receives them, written to path/<name>.npy.
    Whole batch: ICP pose (float32, as computed), status, iterations, extracted and filtered point counts (int32 values,
    stored as float64).  For DUMP_FRAMES frames drawn with a fixed seed: the 0/1 CFAR mask (float32), the float64 points
    and the float32 filtered cloud; the variable-length clouds are concatenated, frame k's rows being
    offsets[k]:offsets[k + 1].  -> total bytes written"""
    n = len(res["status"])
    # python ints: the batch's accessors turn j into a device address offset
    picks = [int(j) for j in np.sort(np.random.default_rng(0).choice(n, min(n, DUMP_FRAMES), replace=False))]
    out = {"icp_T": np.asarray(res["T"], np.float32),
           "icp_status": np.asarray(res["status"], np.float64),
           "icp_iters": np.asarray(res["iters"], np.float64),
           "point_counts": np.asarray(res["counts"], np.float64),
           "sample_frames": np.asarray(picks, np.float64),
           "sample_masks": np.stack([kb.mask(j) for j in picks]).astype(np.float32)}
    pts = [np.asarray(kb.points(j), np.float64).reshape(-1, 2) for j in picks]
    out["sample_points"] = np.concatenate(pts)
    out["sample_points_offsets"] = np.cumsum([0] + [len(p) for p in pts]).astype(np.float64)
    if filters:
        out["cloud_counts"] = np.asarray(res["cloud_counts"], np.float64)
        cl = [np.asarray(kb.cloud(j), np.float32).reshape(-1, 2) for j in picks]
        out["sample_clouds"] = np.concatenate(cl)
        out["sample_clouds_offsets"] = np.cumsum([0] + [len(c) for c in cl]).astype(np.float64)
    total = sum(a.nbytes for a in out.values())
    if total > DUMP_MAX_BYTES:
        raise ValueError("--dump-outputs: %d bytes, more than the %d allowed" % (total, DUMP_MAX_BYTES))
    os.makedirs(path, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(path, name + ".npy"), a)
    return total


def main():
    args = parse()
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        # the legs beyond the timed step, the live-latency leg and the farm leg measure ONE device; in a multi-rank launch
        # they would only keep rank 0's GPU busy for a minute after the line's figure is known (the driver's scaling runs)
        args.no_legs = args.no_latency = args.no_farm = True
    dist = None
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("gloo")  # control plane only; the data path has no collective

    from sonar_slam_amd import _lib, icp_config
    from sonar_slam_amd.CFAR import CFAR
    from sonar_slam_amd.feature_extraction import FeatureExtraction, SonarPing, oculus_bearings
    from sonar_slam_amd.pipeline import KeyframeBatch

    det = CFAR(40, 10, 0.1, 10)                      # feature.yaml:3-7
    frames, srcs, tgts, guesses = make_inputs(rank, args.batch)
    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:   # contract: rank 0 at N=1 only
        # before any HIP call: the worker processes are forked and must not inherit a live GPU context
        from types import SimpleNamespace
        from sonar_slam_amd.feature_extraction import build_maps
        res_, height_, rows_, width_, cols_, map_x_, map_y_ = build_maps(oculus_bearings(COLS), 30.0 / ROWS, ROWS)
        host_fe = SimpleNamespace(map_x=map_x_, map_y=map_y_, rows=rows_, cols=cols_, width=width_, height=height_)
        cpu = cpu_baseline(frames, srcs, tgts, guesses,
                           args.cpu_keyframes, det, host_fe,
                           args.icp_mode, not args.no_filters)
    if args.icp_mode == "p2plane30":
        icp_p = icp_config.shipped_params(minimizer=1, use_diff_checker=0, max_iter=30)
    else:
        icp_p = icp_config.shipped_params()
    # one rank per GPU; SONARFE_BENCH_DEVICE pins every rank to one device (control-plane test on a 1-GPU box).
    # `inflight` resident batches per rank, each with its own context (= its own streams and scratch): a replay that
    # keeps two batches going is how the device stays busy across the serial phases of a step -- the work per step is
    # the same, step k+1 is simply enqueued while step k still runs.
    device = int(os.environ.get("SONARFE_BENCH_DEVICE", local_rank))
    n_inflight = max(1, args.inflight)
    ctxs, fes, kbs = [], [], []
    for _ in range(n_inflight):
        c = _lib.Context(device)
        f = FeatureExtraction(c)
        f.Ntc, f.Ngc, f.Pfa, f.rank, f.alg, f.threshold = 40, 10, 0.1, 10, "SOCA", 65
        f.configure()
        f.generate_map_xy(SonarPing(frames[0], oculus_bearings(COLS), 30.0 / ROWS))
        b = KeyframeBatch(c, f.geometry, det.params["SOCA"], "SOCA", 65, icp_p, args.batch, max_points=args.max_points)
        b.upload_frames(frames)
        b.upload_scan_pairs(srcs, tgts, guesses)
        if not args.serial_prep:
            # the scan pairs are resident and final: the preparation of the ICP targets (sort, strip table, normals)
            # may run on the library's side stream, next to the front-end kernels of the same step (sonarfe.h,
            # sfe_icp_set_tuning bit 3); the iteration kernel waits for both
            c.sync()
            c._check(c.lib.sfe_icp_set_tuning(c.handle, 8))
        b.run(not args.no_filters)   # set-up, not a warm-up step: the context's scratch is allocated on first use
        c.sync()
        ctxs.append(c)
        fes.append(f)
        kbs.append(b)
    ctx, fe, kb = ctxs[0], fes[0], kbs[0]
    # More distinct pings than the 32 the CPU baseline sampled (the data-dependent kernels saw 32 patterns):
    # candidates are generated and screened on the device, untimed -- a ping whose detections exceed the batch's point
    # capacity would be an error on the resident path -- and the batch's frames are re-tiled over the accepted ones.
    n_distinct = min(args.batch, 32)
    n_screened = 0      # candidate pings rejected because their detections exceed the batch's point capacity
    if args.distinct_frames > 32 and args.batch > 32:
        from sonar_slam_amd import synth
        want = min(args.distinct_frames, args.batch)
        accepted = [frames[j] for j in range(32)]
        seed = 1000 * rank + 32
        while len(accepted) < want and seed < 1000 * rank + 32 + 2 * want:
            cand = np.stack([synth.sonar_frame(seed=seed + j) for j in range(min(64, args.batch))])
            seed += len(cand)
            kb.d_img.upload(cand, offset=0)
            kb.run_cfar()
            kb.run_extract()
            ctx.sync()
            cnt = kb.d_cnt.download(np.int32, len(cand))
            accepted += [cand[j] for j in range(len(cand)) if cnt[j] <= kb.cap]
            n_screened += int((cnt > kb.cap).sum())
        accepted = accepted[:want]
        n_distinct = len(accepted)
        frames = np.stack([accepted[j % n_distinct] for j in range(args.batch)])
        for b in kbs:
            b.upload_frames(frames)
            b.run(not args.no_filters)
        for c in ctxs:
            c.sync()

    def barrier():
        for c in ctxs:
            c.sync()
        if dist is not None:
            dist.barrier()

    for i in range(args.warmup):
        kbs[i % n_inflight].run(not args.no_filters)
    barrier()
    t0 = time.perf_counter()
    for i in range(args.steps):
        kbs[(args.warmup + i) % n_inflight].run(not args.no_filters)
    barrier()
    dt = time.perf_counter() - t0
    kb_last = kbs[(args.warmup + args.steps - 1) % n_inflight]   # the batch of the last timed step
    if dist is not None:
        import torch
        t = torch.tensor([dt], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t[0])
    res = kb_last.results()
    ok = int((res["status"] == 0).sum())
    iters_total = int(res["iters"].sum())
    parity = None
    if args.full and rank == 0 and args.parity_jobs > 0:   # the timed step's own outputs, before anything overwrites them
        parity = parity_check(kb_last, res, frames, srcs, tgts, guesses, det, fe, args.icp_mode, not args.no_filters,
                              args.parity_jobs)
    if rank == 0 and args.dump_outputs:      # also before the legs below reuse the batch's buffers
        dump_outputs(args.dump_outputs, kb_last, res, not args.no_filters)

    out = None
    if rank == 0:
        value = args.batch * args.steps * world / dt
        out = {
            "metric": "keyframes/sec (CFAR+ICP) on 512x1024 sonar, 5k-pt pairs",
            "value": value, "unit": "keyframes/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "u8 (CFAR, integer-exact) + f32/f64-accumulate (ICP)", "data": "synthetic",
            "config": {"workload": "BASELINE configs[1]: %d keyframes/step/GPU = 1024x512 SOCA-CFAR(Ntc40,Ngc10)+gate65"
                                   " -> remap+nonzero+px2m%s -> 5000x5000-pt ICP (%s)"
                                   % (args.batch, "" if args.no_filters else " -> downsample 0.5 -> remove_outlier 1.0/5",
                                      args.icp_mode),
                       "batch_per_gpu": args.batch, "distinct_frames": n_distinct, "screened_out_pings": n_screened, "icp_mode": args.icp_mode, "parallelism": "job farm x%d" % world,
                       "icp_prep_stream": "main" if args.serial_prep else "side", "batches_in_flight": n_inflight,
                       "icp_converged_jobs": ok, "mean_icp_iters": iters_total / float(args.batch),
                       "mean_points_per_frame": float(res["counts"].mean()),
                       "max_points_per_frame": int(res["counts"].max()), "points_capacity": kb.cap,
                       "full": args.full}}
    if rank == 0 and args.full:
        # ---- per-stage time and rooflines, HIP events on the stream the kernels run on ----
        def timed(fn, reps):
            fn()
            ctx.sync()
            ctx.timer_start()
            for _ in range(reps):
                fn()
            return ctx.timer_stop() / reps
        ms_cfar_b = timed(kb.run_cfar, 5)
        ms_extract_b = timed(kb.run_extract, 5)
        ms_filter_b = 0.0 if args.no_filters else timed(kb.run_filter, 5)
        # (staged hand-over, round 6: the extraction writes one float32 pair per point for the filters instead of a float64 pair)
        pt_bytes = 8.0 if (kb.staged and not kb.points64) else 16.0
        extract_bytes = float(args.batch) * ROWS * COLS / (8.0 if kb.bit_masks else 1.0) + pt_bytes * float(res["counts"].sum())
        ms_icp_b = timed(kb.run_icp, 2)
        icp_kernel = icp_utilisation(ctx, kb, ms_icp_b, iters_total, args.batch)

        # CFAR roofline leg: a batch larger than the 256 MiB Infinity Cache, one kernel per launch
        nf = args.cfar_frames
        big = ctx.alloc(nf * ROWS * COLS)
        bigm = ctx.alloc(nf * ROWS * COLS)
        for f0 in range(0, nf, args.batch):
            n = min(args.batch, nf - f0)
            big.upload(frames[:n], offset=f0 * ROWS * COLS)
        th, gh, tau = det.params["SOCA"]
        def cfar_big():
            ctx._check(ctx.lib.sfe_cfar_u8_batch_dev(ctx.handle, big.ptr, nf, ROWS, COLS, 1, th, gh, 0, float(tau), 65,
                                                     bigm.ptr, None))
        def cfar_big_bits():
            ctx._check(ctx.lib.sfe_cfar_u8_bits_batch_dev(ctx.handle, big.ptr, nf, ROWS, COLS, 1, th, gh, 0, float(tau),
                                                          65, bigm.ptr))
        def timed_steady(fn, reps, max_warm=400):
            """-> (ms per launch over `reps` launches once the launch time has settled, ms per launch of the first `reps` launches
            after one warm-up call -- what rounds 1-4 reported --, warm-up launches).  The device needs ~100 back-to-back launches
            (~20 ms of load) to reach its sustained clocks: profiles/r05_cfar_series.txt (0.177 ms for launches 25-49, 0.159 from
            launch 125 on); the timed step runs under sustained load, a 20-launch leg after host work does not."""
            first = timed(fn, reps)
            warm, prev = reps + 1, first
            while warm < max_warm:
                cur = timed(fn, 24)
                warm += 25
                if abs(cur - prev) <= 0.01 * prev:
                    break
                prev = cur
            return timed(fn, reps), first, warm
        ms_cfar_bytes, ms_cfar_bytes_first, _ = timed_steady(cfar_big, args.cfar_launches)
        # the algorithmic bytes of the CFAR step are 1 B read + 1 B written per pixel, whatever the kernel
        # does -- `roofline.achieved` is priced on that figure, as the contract asks.  The kernel of the timed step
        # stores the detections as bits (KeyframeBatch.bit_masks): it MOVES 1 B + 1 bit per pixel, less than the
        # algorithmic figure, and is no longer bound by HBM; `moved` prices it on what crosses the pins.
        cfar_bytes = 2.0 * ROWS * COLS * nf
        bits = kb.bit_masks
        ms_cfar, ms_cfar_first, cfar_warm = timed_steady(cfar_big_bits, args.cfar_launches) if bits else (ms_cfar_bytes, ms_cfar_bytes_first, 0)
        cfar_moved = (1.125 if bits else 2.0) * ROWS * COLS * nf
        # ... and the SAME kernel in the shape the timed step launches it (args.batch frames per launch, the batch's own
        # resident frames), under the same warm-up protocol: this is what `roofline.frac` reports from round 6 on (VERDICT r5
        # item 4).  Rounds 1-5 timed this shape over 5 launches after ONE warm-up call and read 0.44 against 0.49 at 1024
        # frames: the difference was the device's clock ramp, not the shape -- at sustained clocks the larger launch is the
        # faster one per frame (profiles/r06_cfar_series.txt: 0.1503 / 0.1476 / 0.1413 us per frame at 1024 / 2048 / 4096).
        ms_cfar_step, ms_cfar_step_first, cfar_step_warm = timed_steady(kb.run_cfar, args.cfar_launches)
        cfar_step_moved = (1.125 if bits else 2.0) * ROWS * COLS * args.batch
        cfar_gbs = cfar_bytes / (ms_cfar * 1e-3) / 1e9
        big.free()
        bigm.free()

        # HBM traffic of the CFAR kernel from the committed PMC passes (rocprofv3 cannot run inside the timed
        # process); only quoted when it was measured on the same launch shape
        traffic, pmc_source = None, None
        pmc_file = "cfar_bits_pmc.json" if bits else "cfar_pmc.json"
        try:
            with open(os.path.join(ROOT, "profiles", pmc_file)) as f:
                pmc = json.load(f)
            if (pmc["frames_per_launch"], pmc["rows"], pmc["cols"]) == (args.batch, ROWS, COLS):
                traffic = pmc["traffic_bytes_per_launch"]
                pmc_source = pmc.get("source_files")
        except (OSError, KeyError, ValueError):
            pass

        extract_traffic = None
        try:
            with open(os.path.join(ROOT, "profiles", "extract_pmc.json")) as f:
                epmc = json.load(f)
            if (epmc["rows"], epmc["cols"]) == (ROWS, COLS):
                extract_traffic = epmc["traffic_bytes_per_frame"] * args.batch
        except (OSError, KeyError, ValueError):
            pass

        # the cloud filters: the extraction's point in (8 B float32 pair staged by the extraction; 16 B float64 on the unstaged
        # path of rounds 2-5) + 8 B out (the float32 point that survives)
        filters_bytes = filters_traffic = None
        if not args.no_filters:
            filters_bytes = (8.0 if kb.staged else 16.0) * float(res["counts"].sum()) + 8.0 * float(res["cloud_counts"].sum())
            try:
                with open(os.path.join(ROOT, "profiles", "filters_pmc.json")) as f:
                    filters_traffic = json.load(f)["traffic_bytes_per_frame"] * args.batch
            except (OSError, KeyError, ValueError):
                pass

        out.update({
            # achieved / frac are priced on the bytes that cross the pins.  The kernel of the timed step
            # stores its detections as bits: per pixel it reads 1 B and writes 1 bit, so ITS algorithmic bytes are 1.125 B
            # per pixel (measured traffic = 1.03 x that), and at that figure it is limited by VALU issue, not by
            # HBM (`limiter`).  SURVEY 8d's 2 B per pixel describe a kernel that writes the byte mask: `frac_survey_bytes`
            # prices the step's CFAR work on that figure, `frac_byte_mask` is the kernel that really moves those bytes
            # (what cfar.soca() of the drop-in returns).  All flat, so that they survive into the driver's record.
            "roofline": {"kernel": "cfar_u8_ring<20,5,SOCA,%s>" % ("BITS" if bits else "bytes"), "bound": "hbm",
                         "limiter": "valu" if bits else "hbm",
                         "limiter_note": ("27 VALU instructions per 256-pixel row and wave, 3 waves per SIMD (168 VGPRs: the ring): ~370 cycles per "
                                          "row against 324 of VALU issue; LDS table latency and the 4-deep load FIFO within 15 % (DESIGN 5.1); "
                                          "round 5: the last tile of a frame runs only the rows it needs (6 % fewer row steps, no change in time)") if bits else "",
                         # achieved / frac: the launch shape of the timed step (args.batch frames per launch, kb.run_cfar), at
                         # sustained clocks: after `warmup_launches` launches whose time had settled within 1 %
                         "achieved": cfar_step_moved / (ms_cfar_step * 1e-3) / 1e9,
                         "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": cfar_step_moved / (ms_cfar_step * 1e-3) / 1e9 / HBM_PEAK_GBS,
                         "traffic": traffic,
                         "traffic_note": "bytes/launch = 2*FETCH_SIZE + WRITE_SIZE from profiles/%s (quoted when that pass ran at "
                                         "this launch shape)" % pmc_file,
                         "bytes_per_launch": cfar_step_moved, "ms_per_launch": ms_cfar_step, "frames_per_launch": args.batch,
                         "frames_per_launch_in_the_step": args.batch,
                         "warmup_launches": cfar_step_warm, "ms_per_launch_first_launches": ms_cfar_step_first,
                         # (the first launches after host work run ~12 % slower -- the clock ramp: what rounds 1-4 put into `frac`)
                         "frac_first_launches": cfar_step_moved / (ms_cfar_step_first * 1e-3) / 1e9 / HBM_PEAK_GBS,
                         # 5 launches after one warm-up call, as the per-stage times below are taken (and as rounds 1-5 reported
                         # `frac_at_step_launch_shape`): mid-ramp
                         "frac_at_step_launch_shape_five_launches_after_one": cfar_step_moved / (ms_cfar_b * 1e-3) / 1e9 / HBM_PEAK_GBS,
                         # the shape rounds 1-5 reported as `frac`: %d frames per launch on a buffer of its own
                         "frac_at_%d_frames_per_launch" % nf: cfar_moved / (ms_cfar * 1e-3) / 1e9 / HBM_PEAK_GBS,
                         "ms_per_launch_at_%d_frames" % nf: ms_cfar, "warmup_launches_at_%d_frames" % nf: cfar_warm,
                         "frac_first_launches_at_%d_frames" % nf: cfar_moved / (ms_cfar_first * 1e-3) / 1e9 / HBM_PEAK_GBS,
                         "bytes_note": "1 B read + %s written per pixel" % ("1 bit" if bits else "1 B"),
                         "achieved_survey_bytes": cfar_gbs, "frac_survey_bytes": cfar_gbs / HBM_PEAK_GBS,
                         "survey_bytes_per_launch": cfar_bytes,
                         "survey_bytes_note": "SURVEY 8d: 1 B read + 1 B written per pixel, priced on the bit-stream kernel's time",
                         "ms_per_launch_byte_mask": ms_cfar_bytes,
                         "achieved_byte_mask": cfar_bytes / (ms_cfar_bytes * 1e-3) / 1e9,
                         "frac_byte_mask": cfar_bytes / (ms_cfar_bytes * 1e-3) / 1e9 / HBM_PEAK_GBS,
                         "counters_from": pmc_source},
            # the ICP kernels prune the search (exact strip-sweep NN): the work below is COUNTED by the kernel in a
            # separate profiled launch of the same batch (sfe_icp_get_profile), not derived from n_src * n_tgt
            "icp_kernel": icp_kernel,
            "stage_ms_per_step": {"cfar": ms_cfar_b, "extract": ms_extract_b, "filters": ms_filter_b, "icp": ms_icp_b},
            "stage_ms_per_512_keyframes": {k: v * 512.0 / args.batch for k, v in
                                           (("cfar", ms_cfar_b), ("extract", ms_extract_b), ("filters", ms_filter_b),
                                            ("icp", ms_icp_b))},
            # SURVEY 8d, on-the-fly form: R*B bytes of mask in + 16 B per extracted point out (8 B on the staged path: float32 pairs)
            "roofline_extract": {"kernel": ("extract_gather<records> + extract_merge_expand (no canvas bitmap in HBM; round 5)" if kb.bit_masks
                                            else "mask_pack + extract_gather + extract_scan + extract_expand_words"), "bound": "hbm",
                                 "limiter": "scattered reads of the inverse-map entries (L1 tag rate: one line per lane and load) and load latency",
                                 "achieved": extract_bytes / (ms_extract_b * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                 "frac": extract_bytes / (ms_extract_b * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                 "bytes_per_launch": extract_bytes, "ms_per_launch": ms_extract_b, "traffic": extract_traffic,
                                 "traffic_note": "bytes/launch from the committed PMC passes (profiles/extract_pmc.json: per-frame "
                                                 "FETCH_SIZE x 2 + WRITE_SIZE of the stage's kernels, scaled to this launch's frames)",
                                 "point_bytes": pt_bytes,
                                 # (rounds 2-5 priced this stage on 16 B per point: the float64 pairs it wrote then.  Writing half the
                                 #  bytes in about the same time LOWERS `frac`; the old pricing is kept next to it for comparison)
                                 "frac_priced_with_float64_points": (float(args.batch) * ROWS * COLS / (8.0 if kb.bit_masks else 1.0) +
                                                                     16.0 * float(res["counts"].sum())) / (ms_extract_b * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                 "note": "algorithmic bytes = the R*B detections (bits when CFAR hands over bit streams) + `point_bytes` per point per frame (16: float64 pairs; 8: the float32 pairs of the staged hand-over to the filters); the kernels are "
                                         "bound by gathers into the inverse remap table (10 MB of 4-byte entries, four candidates per 16-byte read), not "
                                         "by streaming"},
        })
        out["roofline"]["extract_frac"] = out["roofline_extract"]["frac"]      # (flat copies: see the note at `chained` below)
        if filters_bytes is not None:
            out["roofline"]["filters_frac"] = filters_bytes / (ms_filter_b * 1e-3) / 1e9 / HBM_PEAK_GBS
            out["roofline"]["filters_ms_per_launch"] = ms_filter_b
            out["roofline_filters"] = {
                "kernel": ("cf_header_from_bbox + cf_downsample_radix + cf_radius_filter (staged float32 input: no cast pass)" if kb.staged
                           else "cf_cast_bbox + cf_downsample_radix + cf_radius_filter"), "bound": "hbm",
                "limiter": "LDS radix sort and per-leaf medoid loops of the octree downsample: one 1024-thread workgroup and 132 KB of "
                           "LDS per frame (instruction issue at ~55 % VALU-active; profiles/filters_pmc.json)",
                "achieved": filters_bytes / (ms_filter_b * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": filters_bytes / (ms_filter_b * 1e-3) / 1e9 / HBM_PEAK_GBS, "bytes_per_launch": filters_bytes,
                "ms_per_launch": ms_filter_b, "traffic": filters_traffic,
                "bytes_note": "%d B per extracted point in + 8 B per filtered point out (SURVEY 8 f1 / pcl.cpp:128-141,54-74)" % (8 if kb.staged else 16),
                # (as for the extraction: the stage reads half the bytes since round 6, which lowers `frac` at equal time)
                "frac_priced_with_float64_points": (16.0 * float(res["counts"].sum()) + 8.0 * float(res["cloud_counts"].sum())) /
                                                   (ms_filter_b * 1e-3) / 1e9 / HBM_PEAK_GBS,
                "traffic_note": "bytes/launch from the committed PMC passes (profiles/filters_pmc.json), scaled to this launch's frames"}
        try:  # committed SQ counter pass of the ICP loop kernel (rocprofv3 cannot run inside the timed process)
            with open(os.path.join(ROOT, "profiles", "icp_sq.json")) as f:
                sq = json.load(f)
            out["icp_kernel"].update({"valu_active_frac": sq["valu_active_frac"], "wave_wait_frac": sq["wave_wait_frac"],
                                      "counters_from": sq["source"].split(" ")[0], "counters_kernel": sq.get("kernel")})
            if "prep" in sq:
                out["icp_kernel"]["prep_counters"] = sq["prep"]
        except (OSError, KeyError, ValueError):
            pass
        if not args.no_legs:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import bench_legs
            threads = usable_cores()
            small = args.small_legs
            mk = dict(minimizer=1, use_diff_checker=0, max_iter=30) if args.icp_mode == "p2plane30" else {}
            # the 1e-4 bar of north_star against both forms of the oracle, on a sample large enough to show the float
            # oracle's own noise; raises if the HIP path leaves the fp64-sum oracle
            out["float_oracle"] = bench_legs.float_oracle(kb_last, res, srcs, tgts, guesses, mk, threads,
                                                          sample=16 if small else 256)
            out["reference_chain"] = bench_legs.reference_chain(ctx, kb, srcs, tgts, guesses, threads)
            out["stream_frames"] = bench_legs.stream_frames(ctx, kb, not args.no_filters, steps=2 if small else 4,
                                                            distinct=16 if small else 512)
        if not args.no_latency or not args.no_legs:
            for b in kbs:
                b.free()
        if not args.no_legs:
            out["real_size"] = (bench_legs.real_size(ctx, threads, n_ssm=256, n_nssm=8, distinct=64) if small
                                else bench_legs.real_size(ctx, threads))
            out["configs4_hires"] = (bench_legs.configs4_hires(ctx, det, threads, n_pairs=2, n_frames=8, parity_pairs=1) if small
                                     else bench_legs.configs4_hires(ctx, det, threads))
            # the path end to end on the device: every scan match consumes the cloud its own CFAR produced
            out["chained"] = (bench_legs.chained(ctx, det, threads, n_sessions=8, n_steps=4, n_distinct=4, parity_sessions=2, reps=1,
                                                 init_sessions=4, init_parity_sessions=2, init_sessions_one_process=0)
                              if small else bench_legs.chained(ctx, det, threads))
            # the loop-closure search over the store (VERDICT r4 missing 3)
            out["loop_closure"] = (bench_legs.loop_closure(ctx, det, threads, n_keyframes=12, rows=256, beams=128) if small
                                   else bench_legs.loop_closure(ctx, det, threads))
            # (the driver's record keeps `config` and `roofline` whole and only the NAMES of the other keys: the three numbers
            # of these legs a reader will look for first go where they survive)
            out["config"]["chained_keyframes_per_s"] = out["chained"]["keyframes_per_s"]
            out["config"]["chained_with_initialization_keyframes_per_s"] = out["chained"].get("with_initialization", {}).get("keyframes_per_s")
            out["config"]["loop_closure_ms_per_search"] = out["loop_closure"]["ms_per_search_incl_ssm"]
        if not args.no_latency:
            # the live single-item path of the ROS nodes (one ping / one scan match per call, host wall clock incl.
            # PCIe copies and the one synchronisation); the oracle's per-ping / per-match milliseconds are in
            # cpu_baseline.sample
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import live_latency
            # (a live node uses the context as it comes: without the batch pipeline's side-stream preparation, whose event
            # hand-over between two streams costs a single small call ~20 us)
            ctx._check(ctx.lib.sfe_icp_set_tuning(ctx.handle, 0))
            out["live_latency"] = live_latency.measure(ctx)
            out["live_latency"]["note"] = ("median host wall time per call: FeatureExtraction.callback on a 1024x512 ping "
                                           "(fused = sfe_feature_extract_ping, per_stage = the four per-stage calls), "
                                           "pcl.ICP.compute (shipped chain) on n x n points")
        if not args.no_farm:
            out["configs3_farm"] = farm_leg(icp_p, srcs, tgts, guesses, args.farm_jobs)
        if parity is not None:
            out["parity_check"] = parity
        if cpu is not None:
            out["cpu_baseline"] = cpu
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if out is not None:
        print(json.dumps(out))


if __name__ == "__main__":
    main()
