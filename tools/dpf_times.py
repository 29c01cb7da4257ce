"""Times of the ICP chain's data-point filter pass (sfe_icp_dpf.hip) on the bench shape: 4096 jobs of 5000 x 5000
points (distinct clouds), a reading MaxDist stage and a reference octree stage, next to the ICP launch on the filtered
clouds; and the latency a filter chain adds to one 200-point ICP.compute.  Prints one JSON line.

    python tools/dpf_times.py [--jobs 4096] [--reps 5]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sonar_slam_amd import _lib as L  # noqa: E402
from sonar_slam_amd import icp_config, pcl, synth  # noqa: E402

HBM_TBS = 8.0   # MI355X peak HBM bandwidth, TB/s


def stage(kind, dim=-1, f=()):
    st = L.IcpDpf()
    st.kind, st.dim = kind, dim
    for i, v in enumerate(f):
        st.f[i] = v
    return st


def filter_ms(ctx, clouds_flat, off, stages, reps):
    n_cl = len(off) - 1
    d_in = ctx.alloc(clouds_flat.nbytes)
    d_in.upload(clouds_flat)
    d_out = ctx.alloc(clouds_flat.nbytes)
    arr, n = icp_config.IcpChain.device_stages(stages)
    counts = np.zeros(n_cl, np.int32)
    times = []
    for _ in range(reps + 1):
        ctx.sync()
        ctx.timer_start()
        ctx._check(ctx.lib.sfe_icp_filter_clouds_dev(ctx.handle, arr, n, d_in.ptr, L.ptr(off, C.c_int32), n_cl, d_out.ptr,
                                                     L.ptr(counts, C.c_int32)))
        times.append(ctx.timer_stop())
    d_in.free()
    d_out.free()
    return min(times[1:]), counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=4096)
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    ctx = L.default_context()
    pairs = [synth.scan_pair(seed=s, n_src=a.points, n_tgt=a.points) for s in range(16)]
    srcs = [pairs[j % 16][0] for j in range(a.jobs)]
    tgts = [(pairs[j % 16][1] + np.float32(1e-3 * (j // 16))).astype(np.float32) for j in range(a.jobs)]   # distinct
    gs = np.stack([pairs[j % 16][2].reshape(9) for j in range(a.jobs)]).astype(np.float32)
    off = np.arange(a.jobs + 1, dtype=np.int32) * a.points
    rd = [stage(L.DPF_MAX_DIST, -1, [20.0])]
    rf = [stage(L.DPF_OCTREE_GRID, -1, [0.2])]
    src_flat, tgt_flat = np.concatenate(srcs), np.concatenate(tgts)
    ms_rd, c_rd = filter_ms(ctx, src_flat, off, rd, a.reps)
    ms_rf, c_rf = filter_ms(ctx, tgt_flat, off, rf, a.reps)
    bytes_rd = src_flat.nbytes + 8 * int(c_rd.sum())      # read every point, write the kept ones
    out = {"jobs": a.jobs, "points": a.points,
           "reading_maxdist_ms": ms_rd, "reading_kept_mean": float(c_rd.mean()),
           "reading_maxdist_TBs": bytes_rd / ms_rd / 1e9, "reading_maxdist_hbm_frac": bytes_rd / ms_rd / 1e9 / HBM_TBS,
           "reference_octree_ms": ms_rf, "reference_kept_mean": float(c_rf.mean())}
    # the whole call with the chain, and the plain call on clouds filtered beforehand (compute_pairs: host in / out)
    p = icp_config.shipped_params(minimizer=1, use_diff_checker=0, max_iter=30)
    icp = pcl.ICP(ctx)
    icp.setChain(icp_config.IcpChain(p, rd, rf))
    plain = pcl.ICP(ctx)
    plain.setParams(p)
    g3 = [g.reshape(3, 3) for g in gs]
    t_chain, t_plain = [], []
    fs = [srcs[j][np.sqrt(srcs[j][:, 0] ** 2 + srcs[j][:, 1] ** 2) < 20.0] for j in range(a.jobs)]
    ft = [pcl.downsample(t, 0.2, ctx=ctx) for t in tgts]
    for _ in range(2):
        t0 = time.perf_counter()
        r1 = icp.compute_pairs(srcs, tgts, g3)
        t_chain.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        r0 = plain.compute_pairs(fs, ft, g3)
        t_plain.append(time.perf_counter() - t0)
    out["compute_pairs_chain_s"] = min(t_chain)
    out["compute_pairs_prefiltered_s"] = min(t_plain)
    out["compute_pairs_same_status"] = bool(np.array_equal(np.asarray(r1[2]), np.asarray(r0[2])))
    # one 200-point ICP.compute, plain and with a two-sided chain
    src, tgt, guess, _ = synth.scan_pair(seed=99, n_src=200, n_tgt=200)
    sp = icp_config.shipped_params()
    a_icp, b_icp = pcl.ICP(ctx), pcl.ICP(ctx)
    a_icp.setParams(sp)
    b_icp.setChain(icp_config.IcpChain(sp, [stage(L.DPF_MAX_DIST, -1, [40.0])], [stage(L.DPF_MAX_DIST, -1, [40.0])]))
    lat = {}
    for name, obj in (("plain", a_icp), ("chain", b_icp), ("plain2", a_icp), ("chain2", b_icp)):
        ts = []
        for _ in range(200):
            t0 = time.perf_counter()
            obj.compute(src, tgt, guess)
            ts.append(time.perf_counter() - t0)
        lat[name] = float(np.median(ts) * 1e3)
    out["compute200_plain_ms"] = min(lat["plain"], lat["plain2"])
    out["compute200_chain_ms"] = min(lat["chain"], lat["chain2"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
