"""Legs of the bench line beyond the timed BASELINE configs[1] step (bench.py imports this):

  reference_chain   the timed batch's scan pairs through the chain bruce_slam ships (icp.yaml:17-28)
  real_size         the job shapes bruce_slam itself produces (slam.py:769,1032): SSM-like scan matches of 200..1000 points
                    and NSSM batches of 30 guesses x one 800-point pair, small-job tiers vs the 1024-thread kernels
  configs4_hires    BASELINE configs[4]: 2048 x 1024 frames through CFAR + extraction, 20 000-point many-to-one batches
  float_oracle      how often the oracle in float (PointMatcher<float>) is further than 1e-4 from the HIP path, next to
                    its distance from ITSELF with fp64 sums
  stream_frames     the step with its frames arriving from pinned host memory on a copy stream

Every leg that computes poses checks a sample of them against the CPU oracle (as the checker, after its own timed
region) and raises on a mismatch: a line whose work is wrong is not printed."""
import time
from multiprocessing.pool import ThreadPool

import numpy as np

HBM_PEAK_GBS = 8000.0


def pose_diff(Ta, Tb):
    dth = np.arctan2(Ta[1, 0], Ta[0, 0]) - np.arctan2(Tb[1, 0], Tb[0, 0])
    return float(max(abs(Ta[0, 2] - Tb[0, 2]), abs(Ta[1, 2] - Tb[1, 2]), abs(np.arctan2(np.sin(dth), np.cos(dth)))))


def timed(ctx, fn, reps):
    """HIP events on the library's stream around `reps` back-to-back calls (after one untimed call)"""
    fn()
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def oracle_many(jobs, params_kw, threads):
    """[(src, tgt, guess)] -> [(status, T, iters)] for the oracle with fp64 sums and in float, exact kd-tree, on `threads`
    host threads (ctypes releases the GIL; the oracle keeps no shared state besides the kd-tree switch)"""
    import oracle
    oracle.set_kdtree(1)
    try:
        def one(job):
            s, t, g = job
            return (oracle.icp(s, t, g, oracle.shipped_icp_params(precision=1, **params_kw)),
                    oracle.icp(s, t, g, oracle.shipped_icp_params(precision=0, **params_kw)))
        with ThreadPool(max(1, threads)) as tp:
            return tp.map(one, jobs, chunksize=1)
    finally:
        oracle.set_kdtree(0)


def check_against_oracle(name, jobs, got, params_kw, threads, tol64=1e-6):
    """got = (T, status, iters) arrays of `jobs`.  Status and iteration count must equal the oracle with fp64 sums and
    the pose must be within tol64 of it (same discrete decisions); the distance to the oracle in float is reported next
    to that oracle's distance from its own fp64 version."""
    T, status, iters = got
    ref = oracle_many(jobs, params_kw, threads)
    worst64 = worst32 = spread = 0.0
    beyond = 0
    for j, ((st64, T64, it64), (st32, T32, it32)) in enumerate(ref):
        if int(status[j]) != st64 or int(iters[j]) != it64:
            raise AssertionError("%s: job %d status/iterations (%d, %d) vs the oracle's (%d, %d)"
                                 % (name, j, status[j], iters[j], st64, it64))
        if st64 != 0:
            continue
        d64 = pose_diff(T[j], T64)
        if not d64 <= tol64:
            raise AssertionError("%s: job %d pose is %.3e from the oracle (fp64 sums), tolerance %.1e" % (name, j, d64, tol64))
        worst64 = max(worst64, d64)
        if st32 == 0:
            d32 = pose_diff(T[j], T32)
            worst32 = max(worst32, d32)
            spread = max(spread, pose_diff(T32, T64))
            beyond += d32 > 1e-4
    return {"jobs": len(jobs), "max_pose_diff_vs_f64_oracle": worst64, "max_pose_diff_vs_float_oracle": worst32,
            "float_oracle_beyond_1e-4": "%d / %d" % (beyond, len(jobs)),
            "float_oracle_vs_its_own_f64_sums_max": spread}


# ------------------------------------------------------------------------------------------------------------------
def reference_chain(ctx, kb, srcs, tgts, guesses, threads, sample=64):
    """The timed batch's scan pairs through the chain bruce_slam ships: point-to-point, 40-iteration cap, differential
    stop (icp.yaml:17-28) -- the only chain with reference meaning; the headline step runs configs[1]'s 30 forced
    point-to-plane iterations."""
    from sonar_slam_amd import icp_config
    keep = kb.icp_params
    kb.icp_params = icp_config.shipped_params()
    try:
        ms = timed(ctx, kb.run_icp, 3)
        res = kb.results()
    finally:
        kb.icp_params = keep
    n = kb.n
    picks = sorted(set(int(round(i * (n - 1) / max(1, sample - 1))) for i in range(sample)))
    par = check_against_oracle("reference_chain", [(srcs[j], tgts[j], guesses[j]) for j in picks],
                               (res["T"][picks], res["status"][picks], res["iters"][picks]), {}, threads)
    return {"workload": "%d x 5000x5000 scan matches, icp.yaml as shipped (point-to-point, <= 40 iterations, "
                        "differential stop)" % n,
            "ms_per_launch": ms, "jobs_per_s": n / (ms * 1e-3), "mean_iters": float(res["iters"].mean()),
            "converged": int((res["status"] == 0).sum()), "parity": par}


# ------------------------------------------------------------------------------------------------------------------
def real_size(ctx, threads, n_ssm=16384, n_nssm=512, distinct=2048):
    """The jobs bruce_slam produces: feature clouds of 10^2..10^3 points.  SSM-like: independent scan matches
    of 200..1000 x 200..1000 points (slam.py:769); NSSM-like: 30 guesses on one 800 x 800 pair (slam.py:346-358,1032).
    Resident clouds, one launch set per batch; the same batch again with tuning sw_tiers=0 sw_tiny=0 = every job on a
    1024-thread workgroup of the strip sweep (round 2's only shape)."""
    from sonar_slam_amd import icp_config, synth
    from sonar_slam_amd.pipeline import ScanMatchBatch
    rng = np.random.default_rng(11)
    p = icp_config.shipped_params()
    out = {}
    # --- SSM: `distinct` pairs generated, tiled to n_ssm jobs as separate clouds with separate guesses
    sizes = [(int(a), int(b)) for a, b in zip(rng.integers(200, 1001, distinct), rng.integers(200, 1001, distinct))]
    pairs = [synth.scan_pair(seed=5000 + i, n_src=a, n_tgt=b) for i, (a, b) in enumerate(sizes)]
    srcs = [pairs[j % distinct][0] for j in range(n_ssm)]
    tgts = [pairs[j % distinct][1] for j in range(n_ssm)]
    gs = [(pairs[j % distinct][2].astype(np.float64) @ synth.pose_matrix(*rng.normal(0, [0.05, 0.05, 0.005]))).astype(np.float32)
          for j in range(n_ssm)]
    b = ScanMatchBatch(ctx, p, srcs, tgts, [(j, j) for j in range(n_ssm)], gs)
    ms = timed(ctx, b.run, 3)
    res = b.results()
    picks = list(range(0, n_ssm, max(1, n_ssm // 64)))[:64]
    par = check_against_oracle("real_size.ssm", [(srcs[j], tgts[j], gs[j]) for j in picks],
                               (res["T"][picks], res["status"][picks], res["iters"][picks]), {}, threads)
    with ctx.tuning(sw_tiers=0, sw_tiny=0):
        ms_1024 = timed(ctx, b.run, 2)
        res_1024 = b.results()
    same = bool(np.array_equal(res["T"], res_1024["T"]) and np.array_equal(res["iters"], res_1024["iters"]))
    b.free()
    out["ssm"] = {"workload": "%d independent scan matches, 200..1000 x 200..1000 points (%d distinct pairs), icp.yaml as shipped"
                              % (n_ssm, distinct),
                  "ms_per_launch": ms, "jobs_per_s": n_ssm / (ms * 1e-3), "mean_iters": float(res["iters"].mean()),
                  "converged": int((res["status"] == 0).sum()),
                  "all_jobs_on_1024_thread_workgroups": {"ms_per_launch": ms_1024, "jobs_per_s": n_ssm / (ms_1024 * 1e-3),
                                                         "bit_identical_results": same},
                  "speedup_over_1024_thread_workgroups": ms_1024 / ms, "parity": par}
    # --- one size (500 x 500): the figure VERDICT r2 item 2 asks for
    pairs5 = [synth.scan_pair(seed=9000 + i, n_src=500, n_tgt=500) for i in range(1024)]
    n5 = 8192
    b = ScanMatchBatch(ctx, p, [pairs5[j % 1024][0] for j in range(n5)], [pairs5[j % 1024][1] for j in range(n5)],
                       [(j, j) for j in range(n5)], [pairs5[j % 1024][2] for j in range(n5)])
    ms5 = timed(ctx, b.run, 3)
    with ctx.tuning(sw_tiers=0, sw_tiny=0):
        ms5_1024 = timed(ctx, b.run, 2)
    b.free()
    out["at_500_points"] = {"jobs": n5, "jobs_per_s": n5 / (ms5 * 1e-3), "jobs_per_s_1024_thread_workgroups": n5 / (ms5_1024 * 1e-3),
                            "speedup": ms5_1024 / ms5}
    # --- NSSM: 30 guesses per pair
    npair = [synth.scan_pair(seed=7000 + i, n_src=800, n_tgt=800) for i in range(n_nssm)]
    jobs, gs = [], []
    for i, (s, t, g, _) in enumerate(npair):
        for _ in range(30):
            jobs.append((i, i))
            gs.append((g.astype(np.float64) @ synth.pose_matrix(*rng.normal(0, [0.1, 0.1, 0.01]))).astype(np.float32))
    b = ScanMatchBatch(ctx, p, [q[0] for q in npair], [q[1] for q in npair], jobs, gs)
    ms = timed(ctx, b.run, 3)
    res = b.results()
    picks = list(range(0, len(jobs), max(1, len(jobs) // 64)))[:64]
    par = check_against_oracle("real_size.nssm", [(npair[jobs[j][0]][0], npair[jobs[j][1]][1], gs[j]) for j in picks],
                               (res["T"][picks], res["status"][picks], res["iters"][picks]), {}, threads)
    b.free()
    out["nssm"] = {"workload": "%d batches of 30 guesses x one 800x800 pair (slam.py:346-358), icp.yaml as shipped" % n_nssm,
                   "ms_per_launch": ms, "batches_per_s": n_nssm / (ms * 1e-3), "jobs_per_s": len(jobs) / (ms * 1e-3),
                   "mean_iters": float(res["iters"].mean()), "parity": par}
    return out


# ------------------------------------------------------------------------------------------------------------------
def configs4_hires(ctx, det, threads, n_pairs=16, n_frames=256, parity_pairs=2):
    """BASELINE configs[4]: 2048 x 1024 frames (1024 beams x 2048 bins) through CFAR + extraction with the CFAR roofline at
    that shape; the many-to-one ICP batch: 30 guesses (slam.yaml:34) x one 20 000 x 20 000 pair, n_pairs such batches per
    launch, both chains; ONE batch alone = the latency of a loop closure's covariance estimate (slam.py:346-358)."""
    from sonar_slam_amd import icp_config, synth
    from sonar_slam_amd.feature_extraction import FeatureExtraction, SonarPing, oculus_bearings
    from sonar_slam_amd.pipeline import KeyframeBatch, ScanMatchBatch
    ROWS, COLS, NP, NG = 2048, 1024, 20000, 30
    out = {}
    # --- frames
    fe = FeatureExtraction(ctx)
    fe.Ntc, fe.Ngc, fe.Pfa, fe.rank, fe.alg, fe.threshold = 40, 10, 0.1, 10, "SOCA", 65
    fe.configure()
    base = [synth.sonar_frame(seed=300 + s, rows=ROWS, cols=COLS, n_blobs=120) for s in range(16)]
    frames = np.stack([base[j % 16] for j in range(n_frames)])
    fe.generate_map_xy(SonarPing(frames[0], oculus_bearings(COLS), 30.0 / ROWS))
    kb = KeyframeBatch(ctx, fe.geometry, det.params["SOCA"], "SOCA", 65, icp_config.shipped_params(), n_frames, max_points=65536)
    kb.upload_frames(frames)
    ms_cfar = timed(ctx, kb.run_cfar, 10)
    ms_ext = timed(ctx, kb.run_extract, 5)
    counts = kb.results()["counts"]
    import oracle
    th, gh, tau = det.params["SOCA"]
    for j in (0, n_frames - 1):      # two frames against the oracle, bit for bit
        m = oracle.gate(frames[j], oracle.cfar(frames[j], "SOCA", th, gh, tau), 65)
        if not np.array_equal(kb.mask(j), m):
            raise AssertionError("configs4_hires: CFAR mask of frame %d differs from the oracle" % j)
        rc = oracle.nonzero(oracle.remap_u8(m, fe.map_x, fe.map_y))
        if not np.array_equal(kb.points(j), oracle.px_to_m(rc, fe.rows, fe.cols, fe.width, fe.height)):
            raise AssertionError("configs4_hires: extracted points of frame %d differ from the oracle" % j)
    kb.free()
    cfar_bytes = 2.0 * ROWS * COLS * n_frames
    out["frames"] = {"workload": "%d frames 2048x1024 (16 distinct), SOCA-CFAR + gate -> remap + nonzero + px->m" % n_frames,
                     "cfar_ms_per_launch": ms_cfar, "extract_ms_per_launch": ms_ext, "mean_points_per_frame": float(counts.mean()),
                     "roofline": {"kernel": "cfar_u8_ring<20,5,SOCA,BITS>", "bound": "hbm", "bytes_per_launch": cfar_bytes,
                                  "achieved": cfar_bytes / (ms_cfar * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                  "frac": cfar_bytes / (ms_cfar * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                  "note": "SURVEY 8d bytes (1 B read + 1 B written per pixel); the kernel stores bits, "
                                          "so it moves 1.125 B per pixel: x 0.5625 for the bytes that cross the pins"},
                     "frames_bit_exact_vs_oracle": 2}
    # --- many-to-one batches
    rng = np.random.default_rng(4)
    pairs = [synth.scan_pair(seed=400 + i, n_src=NP, n_tgt=NP) for i in range(n_pairs)]
    jobs, gs = [], []
    for i, (s, t, g, _) in enumerate(pairs):
        b0 = synth.pose_of(g)
        for dx, dy, dt in rng.normal(0, [0.3, 0.3, 0.05], (NG, 3)):
            jobs.append((i, i))
            gs.append(synth.pose_matrix(b0[0] + dx, b0[1] + dy, b0[2] + dt).astype(np.float32))
    for name, kw in (("p2plane30", dict(minimizer=1, use_diff_checker=0, max_iter=30)), ("reference_chain", {})):
        p = icp_config.shipped_params(**kw)
        full = ScanMatchBatch(ctx, p, [q[0] for q in pairs], [q[1] for q in pairs], jobs, gs)
        ms_full = timed(ctx, full.run, 2)
        res = full.results()
        full.free()
        one = ScanMatchBatch(ctx, p, [pairs[0][0]], [pairs[0][1]], [(0, 0)] * NG, gs[:NG])
        ms_one = timed(ctx, one.run, 5)
        res_one = one.results()
        with ctx.tuning(sw_multi=0):
            ms_one_unsplit = timed(ctx, one.run, 2)
            res_unsplit = one.results()
        one.free()
        if not (np.array_equal(res_one["iters"], res_unsplit["iters"]) and np.array_equal(res_one["status"], res_unsplit["status"])):
            raise AssertionError("configs4_hires: split and unsplit runs disagree on status / iterations")
        d_split = max(pose_diff(a, b) for a, b in zip(res_one["T"], res_unsplit["T"]))
        # parity: parity_pairs x 30 guesses of the FULL batch against the kd-tree oracle
        pj = [j for j in range(len(jobs)) if jobs[j][0] < parity_pairs]
        par = check_against_oracle("configs4_hires." + name, [(pairs[jobs[j][0]][0], pairs[jobs[j][1]][1], gs[j]) for j in pj],
                                   (res["T"][pj], res["status"][pj], res["iters"][pj]), kw, threads, tol64=1e-5)
        iters = float(res["iters"].sum())
        out[name] = {"workload": "%d batches of %d guesses x one %dx%d pair per launch" % (n_pairs, NG, NP, NP),
                     "ms_per_launch": ms_full, "batches_per_s": n_pairs / (ms_full * 1e-3), "jobs_per_s": len(jobs) / (ms_full * 1e-3),
                     "mean_iters": iters / len(jobs), "converged": int((res["status"] == 0).sum()),
                     "one_batch_ms": ms_one, "one_batch_ms_unsplit": ms_one_unsplit,
                     "one_batch_split_vs_unsplit_max_pose_diff": d_split,
                     "exhaustive_pair_evals_per_launch": float(NP) * NP * iters, "parity": par}
    return out


# ------------------------------------------------------------------------------------------------------------------
def float_oracle(kb, res, srcs, tgts, guesses, params_kw, threads, sample=256):
    """the north_star bar reads 'poses within 1e-4 of the reference CPU path'.  Against the oracle with
    fp64 sums the HIP path agrees to 1e-6 (checked here on `sample` jobs of the timed batch, raising otherwise); the
    oracle in float -- libpointmatcher's own precision -- is itself further than 1e-4 from its fp64 version on about one
    bench-like pair in a hundred (a stop-rule or trimmed-set decision flips on sequential float sums over thousands of
    products), and on exactly those the HIP path differs from it as well."""
    n = kb.n
    picks = sorted(set(int(round(i * (n - 1) / max(1, sample - 1))) for i in range(sample)))
    return check_against_oracle("float_oracle", [(srcs[j], tgts[j], guesses[j]) for j in picks],
                                (res["T"][picks], res["status"][picks], res["iters"][picks]), params_kw, threads)


# ------------------------------------------------------------------------------------------------------------------
def stream_frames(ctx, kb, filters, steps=4, distinct=512, seed0=20000, n_buffers=3, chunk=512, reuse=None, repeats=5):
    """The step with its frames arriving from the host (feature_extraction.py:196-217: every ping does): `distinct`
    frames in pinned memory, uploaded on the context's copy stream in pieces of `chunk` frames into a frame buffer that is
    NOT being computed on (`n_buffers` of them), against the step's kernels on the main stream.  Reports the streamed rate
    next to the resident one of the same loop, the PCIe rate the uploads achieve alone, and how much of the shorter of the
    two is hidden.  Round 5: with THREE buffers the upload of step k + 2 is enqueued behind the CFAR of
    step k -- the only kernel that reads frames, and the last reader of that buffer was the CFAR of step k - 1 -- so the copy
    stream runs without gaps; with two, the upload of step k + 1 had to wait for CFAR(k), which itself queues behind the
    scan matches of step k - 1 (worth ~3 % when the link is in its fast mode)."""
    from sonar_slam_amd import synth
    n, rows, cols = kb.n, kb.rows, kb.cols
    distinct = min(distinct, n)
    frame_b = rows * cols
    fresh = reuse is None or "pool" not in reuse      # (reuse: a dict that carries the pinned pool and the frame buffers from call to call)
    if fresh:
        pool = ctx.host_alloc((distinct, rows, cols), np.uint8)
        for i in range(distinct):
            pool[i] = synth.sonar_frame(seed=seed0 + i, rows=rows, cols=cols)
    else:
        pool = reuse["pool"]
    # the batch stores at most kb.cap points per frame: a frame above it would be truncated (an error on the resident
    # path), so such frames are screened out here -- one untimed pass over the pool, offenders replaced by a neighbour
    replaced = 0
    for f0 in (range(0, distinct, n) if fresh else ()):
        m = min(n, distinct - f0)
        kb.d_img.upload(pool[f0:f0 + m], offset=0)
        kb.run_cfar()
        kb.run_extract()
        ctx.sync()
        cnt = kb.d_cnt.download(np.int32, m)
        good = np.flatnonzero(cnt <= kb.cap)
        for i in np.flatnonzero(cnt > kb.cap):
            pool[f0 + i] = pool[f0 + good[i % len(good)]]
            replaced += 1
    others = reuse["others"] if not fresh else [ctx.alloc(n * frame_b) for _ in range(n_buffers - 1)]       # the other frame buffers
    bufs = [kb.d_img] + others
    chunk = max(1, min(int(chunk), distinct))

    def upload(buf):
        for f0 in range(0, n, chunk):
            m = min(chunk, n - f0)
            p0 = f0 % distinct
            if p0 + m > distinct:
                p0 = 0
            buf.upload_async(pool[p0:p0 + m], offset=f0 * frame_b)

    def step(buf):
        keep = kb.d_img
        kb.d_img = buf
        try:
            kb.run(filters)
        finally:
            kb.d_img = keep

    # the uploads alone
    upload(bufs[0])
    ctx.fence(2)
    t0 = time.perf_counter()
    for k in range(steps):
        upload(bufs[k % n_buffers])
    ctx.fence(2)
    t_copy = (time.perf_counter() - t0) / steps
    # the kernels alone (frames resident: what the headline times)
    step(bufs[0])
    ctx.sync()
    t0 = time.perf_counter()
    for k in range(steps):
        step(bufs[k % n_buffers])
    ctx.sync()
    t_comp = (time.perf_counter() - t0) / steps
    # streamed: the uploads of the next n_buffers - 1 steps are in flight next to the kernels of step k
    ahead = n_buffers - 1

    def streamed():
        for a in range(ahead):
            upload(bufs[a % n_buffers])
        ctx.fence(2)
        ctx.sync()
        t0 = time.perf_counter()
        for k in range(steps):
            # this step's kernels behind this step's upload.  (sfe_stream_fence(0) waits for every upload enqueued SO FAR: with
            # three buffers that includes the one for step k + 1, enqueued a step ago and normally done by now)
            ctx.fence(0)
            kb_buf = bufs[k % n_buffers]
            keep = kb.d_img
            kb.d_img = kb_buf
            try:
                kb.run_cfar()            # the only kernel that reads the frames
                ctx.fence(1)             # the next upload overwrites the buffer CFAR(k + ahead - n_buffers) read: behind CFAR(k)
                upload(bufs[(k + ahead) % n_buffers])   # (also behind the last steps: `steps` uploads inside the timed region)
                kb.run_extract()
                if filters:
                    kb.run_filter()
                kb.run_icp()
            finally:
                kb.d_img = keep
        ctx.sync()
        ctx.fence(2)
        return (time.perf_counter() - t0) / steps
    # The link next to the kernels is BIMODAL on this platform (profiles/r05_stream_probe.txt): ~55 GB/s or ~41 GB/s for whole
    # stretches of seconds, whatever the piece size, the number of buffers or the age of the allocations, while the upload
    # alone always does 57 GB/s.  So the loop is timed `repeats` times and every run is reported; the leg's figure is the MEDIAN.
    runs = sorted(streamed() for _ in range(max(1, repeats)))
    t_stream = runs[len(runs) // 2]
    res = kb.results()
    if reuse is not None:
        reuse["pool"], reuse["others"] = pool, others
    else:
        for o in others:
            o.free()
        ctx.host_free(pool)
    hidden = (t_copy + t_comp - t_stream) / max(1e-12, min(t_copy, t_comp))
    return {"workload": "%d keyframes per step, frames uploaded from pinned host memory (%d distinct frames, %d of them "
                        "replaced by another because they exceed the batch's point capacity; %d MiB per step) in pieces of %d "
                        "frames into %d frame buffers"
                        % (n, distinct, replaced, n * frame_b // (1 << 20), chunk, n_buffers),
            "frame_buffers": n_buffers, "upload_chunk_frames": chunk,
            "keyframes_per_s_streamed": n / t_stream, "keyframes_per_s_resident_same_loop": n / t_comp,
            "ms_per_step_streamed": 1e3 * t_stream, "ms_per_step_resident": 1e3 * t_comp, "ms_upload_alone": 1e3 * t_copy,
            "pcie_gb_per_s_upload_alone": n * frame_b / t_copy / 1e9, "pcie_gb_per_s_while_streaming": n * frame_b / t_stream / 1e9,
            "overlap_fraction": max(0.0, min(1.0, hidden)), "converged": int((res["status"] == 0).sum()),
            "keyframes_per_s_streamed_every_run": [n / t for t in runs], "keyframes_per_s_streamed_best_run": n / runs[0],
            "overlap_fraction_best_run": max(0.0, min(1.0, (t_copy + t_comp - runs[0]) / max(1e-12, min(t_copy, t_comp)))),
            "note": "overlap_fraction = (upload alone + kernels alone - streamed) / min(upload alone, kernels alone); the figures "
                    "are those of the MEDIAN of the streamed runs (the link next to the kernels is bimodal: "
                    "profiles/r05_stream_probe.txt)"}


# ------------------------------------------------------------------------------------------------------------------
def chained_inputs(n_distinct, n_steps, rows=1024, beams=512, world_seed=2, scatterers=3000):
    """`n_distinct` trajectories through ONE synthetic scene (SURVEY 8d Config 2, first option): pings rendered from the
    scene under the true poses, dead-reckoned poses with drifting odometry noise.  Pure numpy: call it before any HIP
    call if it is to fork."""
    from sonar_slam_amd import synth
    from sonar_slam_amd.feature_extraction import oculus_bearings
    # 3000 scatterers: 5-8 k raw detections and 200-300 points per filtered cloud at 1024 x 512 -- the cloud sizes
    # bruce_slam itself produces (10^2..10^3 points)
    world = synth.world_structure(seed=world_seed, n=scatterers)
    bearings = oculus_bearings(beams)
    frames = np.zeros((n_steps, n_distinct, rows, beams), np.uint8)
    dr = np.zeros((n_distinct, n_steps, 3))
    true = np.zeros((n_distinct, n_steps, 3))
    for s in range(n_distinct):
        start = (2.0 + 0.37 * (s % 16), 0.9 * (s // 16) - 2.0 + 0.11 * (s % 5), 0.015 * (s % 9) - 0.06)
        t, d = synth.trajectory(n=n_steps, step=1.7, turn=0.02 + 0.008 * (s % 5), start=start, seed=300 + s)
        true[s], dr[s] = t, d
        for k in range(n_steps):
            frames[k, s] = synth.render_ping(world, t[k], bearings, rows=rows, seed=5000 * s + k)
    return frames, dr, true, bearings


def chained(ctx, det, threads, n_sessions=4096, n_steps=8, n_distinct=64, parity_sessions=None, reps=3, init_sessions=512,
            init_parity_sessions=16, init_sessions_one_process=32):
    """the path end to end on the device, every scan match consuming the cloud its own CFAR produced.
    `n_sessions` independent SLAM sessions advance in lock-step (chained.SessionBatch): step k = ping k of every session
    through CFAR + gate -> remap + nonzero + px->m -> downsample -> outlier filter -> keyframe store -> target cloud =
    get_points(previous <= 3 keyframes under the poses their own scan matches gave them, slam.py:740-741) -> ICP(source,
    target, odometry guess) -> overlap; pings resident in HBM, no cloud crosses PCIe, the host does the SLAM node's
    pose bookkeeping between the calls.  Timed with the host clock around whole runs (the loop has host work in it).
    Parity: `parity_sessions` sessions (default: every distinct one) through the oracle's chain (oracle/chain.py) on the
    same pings.  `with_initialization`: the same path as the reference runs it by DEFAULT (slam.py:77): the shgo global
    initialisation in front of every scan match, its cost function on the device and shgo's decisions replayed for all sessions
    (chained.SessionBatch(initialization=True), shgo_fast.py); `init_sessions` of them also through scipy.optimize.shgo itself,
    record for record the same (shgo is ~8 ms of host Python per scan match)."""
    if parity_sessions is None:
        parity_sessions = n_distinct
    import oracle
    from oracle import chain
    from sonar_slam_amd import chained as ch
    from sonar_slam_amd import icp_config
    from sonar_slam_amd.feature_extraction import FeatureExtraction, SonarPing
    rows, beams = 1024, 512
    t0 = time.perf_counter()
    frames, dr, true, bearings = chained_inputs(n_distinct, n_steps, rows, beams)
    t_render = time.perf_counter() - t0
    fe = FeatureExtraction(ctx)
    fe.Ntc, fe.Ngc, fe.Pfa, fe.rank, fe.alg, fe.threshold = 40, 10, 0.1, 10, "SOCA", 65
    fe.configure()
    fe.generate_map_xy(SonarPing(frames[0, 0], bearings, 30.0 / rows))
    sel = np.arange(n_sessions) % n_distinct
    out = {"workload": "%d sessions x %d keyframes (%d distinct trajectories through one synthetic scene, 1024x512 pings, "
                       "1.7 m apart, drifting odometry): CFAR -> cloud -> store -> get_points(last 3) -> ICP -> overlap, "
                       "device-resident" % (n_sessions, n_steps, n_distinct),
           "sessions": n_sessions, "keyframes_per_session": n_steps, "distinct_sessions": n_distinct,
           "replication": "%d distinct trajectories x %d copies: the copies do identical work on identical pings (they share "
                          "nothing on the device, but their inverse-map / table reads hit the same cache lines)"
                          % (n_distinct, n_sessions // max(1, n_distinct)),
           "render_s": t_render}
    # the pings go up once (n_sessions x n_steps x 512 KB resident: 16 GB at the default size) and serve both chains
    sb = ch.SessionBatch(ctx, fe.geometry, det.params["SOCA"], "SOCA", 65, icp_config.shipped_params(), n_sessions, n_steps,
                         dr[sel])
    for k in range(n_steps):
        sb.upload_frames(k, frames[k][sel])
    for name, params in (("shipped_chain", icp_config.shipped_params()),
                         ("p2plane30", icp_config.shipped_params(minimizer=1, use_diff_checker=0, max_iter=30))):
        sb.icp_params = params
        sb.run()                                # untimed: scratch and store allocations
        out["points_capacity"] = sb.fit_capacity()      # (sized by the largest ping of the warm-up run)
        out["max_raw_points_per_ping"] = sb.max_raw
        sb.run()
        ctx.sync()
        best = None
        for _ in range(reps):
            ctx.sync()
            t0 = time.perf_counter()
            recs = sb.run()
            ctx.sync()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        status = np.stack([r["status"] for r in recs[1:]], axis=1)           # [S x (K-1)]
        n_src = np.stack([r["n_source"] for r in recs], axis=1)
        n_tgt = np.stack([r["n_target"] for r in recs[1:]], axis=1)
        iters = np.stack([r["iters"] for r in recs[1:]], axis=1)
        est = np.stack([r["pose"] for r in recs], axis=1)                    # [S x K x 3]

        def end_error(p):       # relative motion first -> last keyframe against ground truth (the frames differ by a
            e = []              # constant: sensor frame vs world frame)
            for s in range(n_distinct):
                a, b, ta, tb = chain.pose(*p[s, 0]), chain.pose(*p[s, -1]), chain.pose(*true[s, 0]), chain.pose(*true[s, -1])
                got, want = chain.between(a, b), chain.between(ta, tb)
                e.append(np.hypot(got[0] - want[0], got[1] - want[1]))
            return float(np.mean(e)), float(np.max(e))
        leg = {"seconds_per_run": best, "keyframes_per_s": n_sessions * n_steps / best,
               "scan_matches_per_s": n_sessions * (n_steps - 1) / best, "ms_per_step": 1e3 * best / n_steps,
               "status_counts": {ch.STATUS_NAMES[c]: int((status == c).sum()) for c in range(1, 6) if (status == c).any()},
               "mean_source_points": float(n_src.mean()), "mean_target_points": float(n_tgt.mean()),
               "mean_icp_iters": float(iters[status != ch.NOT_ENOUGH_POINTS].mean()),
               "end_position_error_m": dict(zip(("icp_chain_mean", "icp_chain_max"), end_error(est[:n_distinct]))),
               "odometry_end_position_error_m": dict(zip(("mean", "max"), end_error(dr)))}
        # ---- parity: whole sessions through the oracle's chain (feature cloud, target cloud, ICP, overlap, pose) ----
        picks = sorted(set(int(round(i * (n_distinct - 1) / max(1, parity_sessions - 1))) for i in range(parity_sessions)))
        oprm = oracle.IcpParams(precision=1, **params.as_dict())
        oracle.set_kdtree(1)
        try:
            def one(s):
                clouds = [chain.slam_cloud(chain.feature_cloud(frames[k, s], det.params["SOCA"], "SOCA", 65, fe)[1])
                          for k in range(n_steps)]
                return clouds, chain.run_session(clouds, dr[s], oprm)
            with ThreadPool(max(1, threads)) as tp:
                ref = tp.map(one, picks, chunksize=1)
        finally:
            oracle.set_kdtree(0)
        worst = 0.0
        for s, (clouds, orc) in zip(picks, ref):
            if not np.array_equal(sb.store.read(sb.handles[s, n_steps - 1]), clouds[-1]):
                raise AssertionError("chained/%s: session %d, the stored cloud of the last keyframe differs from the oracle's" % (name, s))
            for k, o in enumerate(orc):
                r = recs[k]
                if ch.STATUS_NAMES[r["status"][s]] != o["status"] or r["n_source"][s] != o["n_source"]:
                    raise AssertionError("chained/%s: session %d keyframe %d: %s / %d points vs the oracle's %s / %d"
                                         % (name, s, k, ch.STATUS_NAMES[r["status"][s]], r["n_source"][s], o["status"], o["n_source"]))
                if k and (r["n_target"][s] != o["n_target"] or ("icp_status" in o and (r["icp_status"][s] != o["icp_status"]
                                                                                        or r["iters"][s] != o["iters"]))
                          or ("overlap" in o and r["overlap"][s] != o["overlap"])):
                    raise AssertionError("chained/%s: session %d keyframe %d differs from the oracle chain" % (name, s, k))
                d = max(abs(a - b) for a, b in zip(r["pose"][s], o["pose"]))
                if not d <= 1e-6:
                    raise AssertionError("chained/%s: session %d keyframe %d pose is %.3e from the oracle chain" % (name, s, k, d))
                worst = max(worst, d)
        leg["parity"] = {"sessions": picks, "keyframes": len(picks) * n_steps, "max_pose_diff_vs_oracle_chain": worst,
                         "checked": "per keyframe: status, source / target cloud sizes, ICP status and iteration count, "
                                    "overlap (equal), pose <= 1e-6 vs oracle/chain.py (fp64-sum ICP, exact kd-tree); last "
                                    "keyframe's stored cloud bit-exact"}
        out[name] = leg
    sb.free()
    out["keyframes_per_s"] = out["shipped_chain"]["keyframes_per_s"]
    # ---- the reference's default flow: shgo global initialisation in front of every scan match ----
    if init_sessions:
        def timed_init(S, workers, replay):
            sel_i = np.arange(S) % n_distinct
            sbi = ch.SessionBatch(ctx, fe.geometry, det.params["SOCA"], "SOCA", 65, icp_config.shipped_params(), S, n_steps, dr[sel_i],
                                  initialization=True, shgo_workers=workers, shgo_replay=replay)
            for k in range(n_steps):
                sbi.upload_frames(k, frames[k][sel_i])
            sbi.run()                           # untimed: scratch, store, the plan / the Sobol set, the worker processes
            sbi.fit_capacity()
            for key in sbi.init_stats:
                sbi.init_stats[key] = 0
            ctx.sync()
            t0 = time.perf_counter()
            recs = sbi.run()
            ctx.sync()
            return sbi, recs, time.perf_counter() - t0
        # scipy.optimize.shgo per session (the way of this round's first half): on the host cores, and on one process
        S0 = int(init_sessions)
        sb0, recs0, dt0 = timed_init(S0, max(1, threads), False)
        scipy_only = {"sessions": S0, "shgo_worker_processes": max(1, threads), "keyframes_per_s": S0 * n_steps / dt0,
                      "host_shgo_share": sb0.init_stats["shgo_s"] / dt0,
                      "speculative_runs": sb0.init_stats["speculated"], "speculative_runs_redone": sb0.init_stats["speculation_failed"]}
        sb0.free()
        if init_sessions_one_process and threads > 1:
            sb1, _, dt1 = timed_init(int(init_sessions_one_process), 1, False)
            scipy_only["one_process"] = {"sessions": int(init_sessions_one_process),
                                         "keyframes_per_s": init_sessions_one_process * n_steps / dt1,
                                         "host_shgo_share": sb1.init_stats["shgo_s"] / dt1}
            sb1.free()
        # ... and with shgo's decisions replayed from one table of costs per step (shgo_fast.py), scipy only where the replay
        # reports a session as undecidable
        S = int(n_sessions)
        sbi, recs, dt = timed_init(S, max(1, threads), True)
        status = np.stack([r["status"] for r in recs[1:]], axis=1)
        moved = np.stack([np.any(r["init_x"] != 0, axis=1) for r in recs[1:] if "init_x" in r], axis=1)
        # the replay against scipy inside the product: the first S0 sessions of both runs are the same sessions
        n_same = 0
        for r, r0 in zip(recs, recs0):
            for key in ("status", "init_success", "init_x", "init_cost", "pose", "transform", "overlap"):
                if key in r0 and not np.array_equal(r[key][:S0], r0[key]):
                    bad = int(np.nonzero((np.asarray(r[key][:S0]) != np.asarray(r0[key])).reshape(S0, -1).any(axis=1))[0][0])
                    raise AssertionError("chained/with_initialization: step %d session %d: %s differs between the replayed shgo and "
                                         "scipy.optimize.shgo: %r vs %r" % (r["k"], bad, key, r[key][bad], r0[key][bad]))
            n_same += S0 if "init_x" in r0 else 0
        # the figure under this key is the rate WITH the replays: a scipy that switched them off must not print the scipy-only
        # rate in its place
        from sonar_slam_amd import shgo_fast
        replay_status = shgo_fast.status()
        if sbi.init_stats["replayed"] == 0 or not any(v["active"] for v in replay_status["replays"].values()):
            raise AssertionError("chained/with_initialization: the shgo replays are OFF for scipy %s (shgo_fast.py was developed "
                                 "against %s): %r -- this leg would report the scipy-only rate under the replay's key"
                                 % (replay_status["scipy"], replay_status["developed_against"], replay_status["replays"]))
        leg = {"sessions": S, "seconds_per_run": dt, "keyframes_per_s": S * n_steps / dt,
               "shgo_replays": replay_status,
               "ms_per_scan_match": 1e3 * dt / (S * (n_steps - 1)),
               "host_seconds_after_the_cost_table": sbi.init_stats["shgo_s"], "host_share": sbi.init_stats["shgo_s"] / dt,
               "seconds_sample_transforms_on_the_host": sbi.init_stats["transforms_s"],
               "seconds_cost_grids_built": sbi.init_stats["grids_s"], "seconds_cost_table_launches": sbi.init_stats["table_s"],
               "scan_matches_replayed": sbi.init_stats["replayed"], "scan_matches_handed_to_scipy": sbi.init_stats["replay_fallbacks"],
               "cost_evaluations_from_the_batched_table": sbi.init_stats["table_hits"],
               "cost_evaluations_verified_afterwards": sbi.init_stats["cost_calls"],
               "scan_matches_equal_to_the_scipy_only_run": n_same,
               "scipy_only": scipy_only,
               "scan_matches_whose_start_shgo_moved": int(moved.sum()),
               "status_counts": {ch.STATUS_NAMES[c]: int((status == c).sum()) for c in range(1, 7) if (status == c).any()},
               "note": "slam.py:665-716 per scan match.  The cost at shgo's 61 sampling vertices and at the 3 finite-difference points "
                       "SLSQP adds per vertex is taken for ALL sessions in one launch (sfe_matching_cost_store_samples: the sample transforms computed on the device, 244 poses per "
                       "session); what shgo decides from there (minimiser pool, order of the local minimisations, result) is "
                       "replayed by sfe_shgo_sobol_replay from the graph of ONE run of the installed scipy (shgo_fast.py); a session "
                       "whose finite-difference point lands in another cell, or with an exact distance tie, goes through "
                       "scipy.optimize.shgo itself.  `scipy_only`: every session through scipy.optimize.shgo on the host cores "
                       "(shgo_pool.py) -- the same records, compared above"}
        picks = sorted(set(int(round(i * (min(S, n_distinct) - 1) / max(1, init_parity_sessions - 1))) for i in range(init_parity_sessions)))
        oprm = oracle.IcpParams(precision=1, **icp_config.shipped_params().as_dict())
        oracle.set_kdtree(1)
        try:
            def one_i(s):
                clouds = [chain.slam_cloud(chain.feature_cloud(frames[k, s], det.params["SOCA"], "SOCA", 65, fe)[1]) for k in range(n_steps)]
                return chain.run_session(clouds, dr[s], oprm, initialization=True)
            with ThreadPool(max(1, threads)) as tp:
                ref = tp.map(one_i, picks, chunksize=1)
        finally:
            oracle.set_kdtree(0)
        worst = 0.0
        for s, orc in zip(picks, ref):
            for k, o in enumerate(orc):
                r = recs[k]
                if ch.STATUS_NAMES[r["status"][s]] != o["status"]:
                    raise AssertionError("chained/with_initialization: session %d keyframe %d: %s vs the oracle's %s"
                                         % (s, k, ch.STATUS_NAMES[r["status"][s]], o["status"]))
                if "init_x" in o and (tuple(r["init_x"][s]) != o["init_x"] or r["init_cost"][s] != o["init_cost"]):
                    raise AssertionError("chained/with_initialization: session %d keyframe %d: shgo found %r (%g), the oracle chain %r (%g)"
                                         % (s, k, tuple(r["init_x"][s]), r["init_cost"][s], o["init_x"], o["init_cost"]))
                d = max(abs(a - b) for a, b in zip(r["pose"][s], o["pose"]))
                if not d <= 1e-6:
                    raise AssertionError("chained/with_initialization: session %d keyframe %d pose is %.3e from the oracle chain" % (s, k, d))
                worst = max(worst, d)
        leg["parity"] = {"sessions": picks, "max_pose_diff_vs_oracle_chain": worst,
                         "checked": "per keyframe: status, shgo's result x and value (equal), pose <= 1e-6 vs oracle/chain.py with "
                                    "initialization=True (CPU cost function + the same scipy shgo)"}
        out["with_initialization"] = leg
        sbi.free()
    return out


def loop_closure(ctx, det, threads, n_keyframes=14, rows=1024, beams=512, world_seed=2, scatterers=9000):
    """The loop-closure search of slam.py:839-1087 over the device-resident keyframe store (VERDICT r4 missing 3): one
    session on a closed trajectory (13 keyframes per lap), replay.FrontEnd(store, nssm_enable=True): after every keyframe the
    aggregated source cloud, the keyed global target cloud of every keyframe older than k - 8 (descriptor overload of
    pcl.downsample), the field-of-view gate, shgo (100 x 5) on the device cost function -- its decisions replayed from ONE launch
    over every point that can become a vertex (shgo_fast.replay_multi) -- the target-key refinement, <= 30 ICPs on one pair in
    one launch, MinCovDet, the gates.  Parity: the whole session through oracle/chain.py (initialization + nssm, scipy's shgo),
    and against the same front end with scipy.optimize.shgo in the loop."""
    import oracle
    from oracle import chain
    from sonar_slam_amd import icp_config, synth
    from sonar_slam_amd import store as st
    from sonar_slam_amd.feature_extraction import FeatureExtraction, SonarPing, oculus_bearings
    from sonar_slam_amd.replay import FrontEnd, replay
    bearings = oculus_bearings(beams)
    world = synth.world_structure(seed=world_seed, n=scatterers)
    true, dr = synth.trajectory(n=n_keyframes, step=1.7, turn=2 * np.pi / 13, seed=21, start=(20.0, 0.0, 0.0))
    frames = [synth.render_ping(world, true[k], bearings, rows=rows, seed=7000 + k) for k in range(n_keyframes)]
    fe = FeatureExtraction(ctx)
    fe.Ntc, fe.Ngc, fe.Pfa, fe.rank, fe.alg, fe.threshold = 40, 10, 0.1, 10, "SOCA", 65
    fe.resolution, fe.outlier_filter_radius, fe.outlier_filter_min_points, fe.skip = 0.5, 1.0, 5, 1
    fe.configure()
    pings = [SonarPing(f, bearings, 30.0 / rows, ping_id=k) for k, f in enumerate(frames)]
    fe.generate_map_xy(pings[0])

    def run(shgo_replay):
        s = st.CloudStore(ctx, capacity_points=1 << 20, max_clouds=1024)
        front = FrontEnd(ctx, keyframe_translation=1.5, keyframe_duration=0.5, store=s, nssm_enable=True, mcd_random_state=0,
                         shgo_replay=shgo_replay)
        t0 = time.perf_counter()
        log, t_fe, t_slam = replay(pings, np.arange(n_keyframes, dtype=float), dr, fe, front)
        dt = time.perf_counter() - t0
        s.close()
        return front, log, dt, t_fe, t_slam
    # the replays of shgo's decisions are checked against the installed scipy once per process: not part of the timed session
    from sonar_slam_amd import shgo_fast
    pose_stds = np.array([[0.2, 0.2, 0.02]]).T
    plan = shgo_fast.plan_for(5.0 * np.c_[-pose_stds, pose_stds], 50, 0.01)
    if plan.checked is None:
        plan.self_check()
    shgo_fast.multi_checked(100, 5, 0.01)
    front, log, dt, t_fe, t_slam = run(True)
    _, log_scipy, dt_scipy, _, t_slam_scipy = run(False)       # scipy.optimize.shgo for every initialisation: the same records
    for a, b in zip(log, log_scipy):
        na, nb = dict(a.get("nssm") or {}), dict(b.get("nssm") or {})
        na.pop("init_replayed", None)
        nb.pop("init_replayed", None)
        same = a["status"] == b["status"] and a["pose"] == b["pose"] and set(na) == set(nb) and all(
            np.array_equal(np.asarray(na[k]), np.asarray(nb[k])) for k in na)
        if not same:
            raise AssertionError("loop_closure: keyframe %d differs between the replayed shgo and scipy.optimize.shgo" % a["source_key"])
    searches = [r["nssm"] for r in log if r.get("nssm") is not None]
    clouds = [chain.slam_cloud(chain.feature_cloud(f, det.params["SOCA"], "SOCA", 65, fe)[1]) for f in frames]
    oracle.set_kdtree(1)
    try:
        t0 = time.perf_counter()
        orc = chain.run_session(clouds, dr, oracle.IcpParams(precision=1, **icp_config.shipped_params().as_dict()), initialization=True,
                                nssm=dict(mcd_random_state=0))
        t_oracle = time.perf_counter() - t0
    finally:
        oracle.set_kdtree(0)
    n_checked = 0
    for a, o in zip(log, orc):
        na, no = a.get("nssm"), o.get("nssm")
        if (na is None) != (no is None):
            raise AssertionError("loop_closure: keyframe %d: a search on one side only" % a["source_key"])
        if a["status"] != o["status"] or max(abs(x - y) for x, y in zip(a["pose"], o["pose"])) > 1e-6:
            raise AssertionError("loop_closure: keyframe %d: sequential scan match differs from the oracle chain" % a["source_key"])
        if na is None:
            continue
        for key in ("status", "n_source", "n_target_global", "target_key_fov", "init_x", "init_cost", "overlap_global", "target_key",
                    "n_target", "n_guesses", "n_converged", "overlap"):
            if (key in na) != (key in no) or (key in na and na[key] != no[key]):
                raise AssertionError("loop_closure: keyframe %d: %s = %r, the oracle chain has %r" % (a["source_key"], key, na.get(key), no.get(key)))
        if "transform" in no and max(abs(x - y) for x, y in zip(na["transform"], no["transform"])) > 1e-6:
            raise AssertionError("loop_closure: keyframe %d: loop transform differs from the oracle chain" % a["source_key"])
        n_checked += 1
    status = {}
    for n in searches:
        status[n["status"]] = status.get(n["status"], 0) + 1
    return {"workload": "1 session, %d keyframes %dx%d on a closed trajectory (13 per lap): SSM with global initialisation + the "
                        "loop-closure search after every keyframe >= 8, all clouds device-resident" % (n_keyframes, rows, beams),
            "searches": len(searches), "status_counts": status, "accepted_loops": status.get("SUCCESS", 0),
            "seconds_per_session": dt, "ms_per_keyframe_front_end": 1e3 * t_fe / n_keyframes,
            "ms_per_keyframe_slam_side": 1e3 * t_slam / n_keyframes, "ms_per_search_incl_ssm": 1e3 * t_slam / max(1, len(searches)),
            "searches_whose_shgo_was_replayed": sum(bool(n.get("init_replayed")) for n in searches),
            "scipy_only": {"seconds_per_session": dt_scipy, "ms_per_search_incl_ssm": 1e3 * t_slam_scipy / max(1, len(searches)),
                           "note": "scipy.optimize.shgo itself for every initialisation (FrontEnd(shgo_replay=False)): the records "
                                   "of the two runs are compared field by field"},
            "largest_global_target_points": max([n.get("n_target_global", 0) for n in searches] + [0]),
            "largest_icp_target_points": max([n.get("n_target", 0) for n in searches] + [0]),
            "oracle_chain_seconds": t_oracle,
            "parity": {"searches": n_checked, "checked": "per search: status, cloud sizes, field-of-view target key, shgo's x and value, "
                                                         "refined target key, number of guesses / converged ICPs, overlap (equal); loop "
                                                         "transform <= 1e-6 vs oracle/chain.py"},
            "note": "PCM (slam.py:1089-1130) and the ISAM2 update are the back end: an accepted loop goes to backend.add_loop"}
