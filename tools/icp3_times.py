"""Wall time of ``pcl.ICP`` on N x 3 clouds with 4 x 4 guesses (sfe_icp3.hip): host arrays in, host arrays out, so copies
and launch latencies are included.  Three shapes: a single ``compute`` and a ``compute_batch`` of 30 guesses on an 800 x 800
pair (the loop of SLAM.compute_icp_with_cov), and ``compute_pairs`` on 256 pairs of 5000 x 5000.  The same calls on the
(x, y) columns of the same clouds stand next to them.  Medians over --reps calls after two warm-up calls; one JSON line.

    python tools/icp3_times.py [--reps 9] [--pairs 256] [--n 5000]

``--minimizer plane`` times the 3-D calls with the point-to-plane minimiser (``minimizer = 2``) instead, ``--minimizer both``
alternates the two minimisers call by call in one process and prints every repeat (``series``), the medians, the ratio plane /
point, and ``pcl.surface_normals`` alone on one target of either size (a host call: the copy up, the normals kernel, the copy
down) with its share of the plane time of ``compute`` and of the 30 guesses, which have one distinct target each; the normals
of the 256 targets of ``compute_pairs`` are one launch, whose share is read from a kernel trace
(``rocprofv3 --kernel-trace -- python tools/icp3_times.py --minimizer plane``).  ``--minimizer point`` (the default) prints
what the tool always printed.  ``--minimizer 4dof`` alternates the point-to-plane minimiser with its 4-DoF form (``minimizer = 3``:
yaw and translation only) in the same way, on the same pairs, and prints the range of every series and the ratio 4dof / plane.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sonar_slam_amd import _lib, icp_config, pcl  # noqa: E402


def med_ms(f, reps):
    for _ in range(2):
        f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return round(1e3 * float(np.median(t)), 4)


def rigid(axis, angle, t):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    T[:3, 3] = t
    return T


def pair(rng, n, truth):
    """a cloud of n points in a 30 x 30 x 10 m box and the same points, noisy, seen from a frame ``truth`` maps back"""
    world = rng.uniform(-1, 1, (n, 3)) * np.array([15.0, 15.0, 5.0])
    tgt = world + rng.normal(0, 0.02, (n, 3))
    src = world[rng.permutation(n)] + rng.normal(0, 0.02, (n, 3))
    Ti = np.linalg.inv(truth)
    return (src @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32), tgt.astype(np.float32)


def planar(T4):
    T3 = np.eye(3, dtype=np.float32)
    T3[:2, :2] = T4[:2, :2]
    T3[:2, 2] = T4[:2, 3]
    return T3


def minimizers(ctx, a, s, t, guess, guesses, big, out):
    """the three 3-D shapes with the point-to-plane minimiser, alone or alternated with point-to-point, or (``4dof``)
    alternated with its 4-DoF form"""
    kinds = {"point": 0, "plane": 2}
    if a.minimizer == "plane":
        kinds.pop("point")
    elif a.minimizer == "4dof":
        kinds = {"plane": 2, "4dof": 3}
    icps = {}
    for k, m in kinds.items():
        icps[k] = pcl.ICP(ctx)
        icps[k].setParams(icp_config.shipped_params(minimizer=m))
    srcs, tgts, gb = [p[0] for p in big], [p[1] for p in big], [guess] * len(big)
    pairs_name = "compute_pairs_%d_x_%dx%d" % (a.pairs, a.n, a.n)
    shapes = (("compute_800x800", lambda i: i.compute(s, t, guess), a.reps),
              ("compute_batch_30_guesses_800x800", lambda i: i.compute_batch(s, t, guesses), a.reps),
              (pairs_name, lambda i: i.compute_pairs(srcs, tgts, gb), max(a.reps // 3, 5 if len(kinds) == 2 else 1)))
    out.update({"minimizer": a.minimizer, "series": {k: {} for k in kinds}, "ms": {k: {} for k in kinds}})
    for name, call, reps in shapes:
        ser = {k: [] for k in kinds}
        for r in range(reps + 2):                      # two warm-up rounds, then alternate call by call
            for k in kinds:
                t0 = time.perf_counter()
                call(icps[k])
                if r >= 2:
                    ser[k].append(round(1e3 * (time.perf_counter() - t0), 4))
        for k in kinds:
            out["series"][k][name] = ser[k]
            out["ms"][k][name] = round(float(np.median(ser[k])), 4)
    for k in kinds:
        msgs, _, it = icps[k].compute_pairs(srcs, tgts, gb)
        out["iterations"][k] = {"pairs_mean": round(float(np.mean(it)), 2), "pairs_success": int(sum(m == "success" for m in msgs)),
                                "batch_mean": round(float(np.mean(icps[k].compute_batch(s, t, guesses)[2])), 2)}
    knn = icp_config.shipped_params().normals_knn
    nrm = {"surface_normals_800": med_ms(lambda: pcl.surface_normals(t, knn, ctx=ctx), a.reps),
           "surface_normals_%d" % a.n: med_ms(lambda: pcl.surface_normals(big[0][1], knn, ctx=ctx), a.reps)}
    out["normals_ms"] = nrm
    ms = out["ms"]["plane"]
    out["normals_share"] = {"compute_800x800": round(nrm["surface_normals_800"] / ms["compute_800x800"], 3),
                            "compute_batch_30_guesses_800x800": round(nrm["surface_normals_800"] / ms["compute_batch_30_guesses_800x800"], 3),
                            }  # (the pairs' normals run as one launch over all targets: their share is read from a kernel trace)
    if "point" in kinds:
        out["plane_over_point"] = {n: round(ms[n] / out["ms"]["point"][n], 3) for n in ms}
    if "4dof" in kinds:
        out["range_ms"] = {k: {n: [min(v), max(v)] for n, v in out["series"][k].items()} for k in kinds}
        out["4dof_over_plane"] = {n: round(out["ms"]["4dof"][n] / ms[n], 3) for n in ms}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--minimizer", choices=("point", "plane", "both", "4dof"), default="point")
    a = ap.parse_args()
    ctx = _lib.default_context()
    icp = pcl.ICP(ctx)
    icp.setParams(icp_config.shipped_params())
    rng = np.random.default_rng(1)
    # rotations about z, so that the (x, y) columns are a 2-D job of the same difficulty
    truth = rigid((0, 0, 1), 0.087, (0.8, -0.3, 0.0))
    guess = np.asarray(rigid((0, 0, 1), 0.052, (0.3, -0.2, 0.0)) @ truth, np.float32)
    s, t = pair(rng, 800, truth)
    guesses = [np.asarray(rigid((0, 0, 1), rng.uniform(-0.05, 0.05), np.r_[rng.uniform(-0.3, 0.3, 2), 0]) @ truth, np.float32)
               for _ in range(30)]
    big = [pair(rng, a.n, truth) for _ in range(a.pairs)]
    out = {"tool": "icp3_times", "device": ctx.name(), "reps": a.reps, "ms": {}, "iterations": {}}
    if a.minimizer != "point":
        print(json.dumps(minimizers(ctx, a, s, t, guess, guesses, big, out)))
        return
    for name, cut, g_of in (("3d", lambda c: c, lambda g: g), ("2d", lambda c: np.ascontiguousarray(c[:, :2]), planar)):
        s1, t1 = cut(s), cut(t)
        srcs, tgts = [cut(p[0]) for p in big], [cut(p[1]) for p in big]
        gs, gb = [g_of(g) for g in guesses], [g_of(guess)] * len(big)
        out["ms"][name] = {
            "compute_800x800": med_ms(lambda: icp.compute(s1, t1, g_of(guess)), a.reps),
            "compute_batch_30_guesses_800x800": med_ms(lambda: icp.compute_batch(s1, t1, gs), a.reps),
            "compute_pairs_%d_x_%dx%d" % (a.pairs, a.n, a.n): med_ms(lambda: icp.compute_pairs(srcs, tgts, gb), max(a.reps // 3, 1)),
        }
        msgs, _, it = icp.compute_pairs(srcs, tgts, gb)
        out["iterations"][name] = {"pairs_mean": round(float(np.mean(it)), 2), "pairs_success": int(sum(m == "success" for m in msgs)),
                                   "batch_mean": round(float(np.mean(icp.compute_batch(s1, t1, gs)[2])), 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
