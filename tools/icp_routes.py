#!/usr/bin/env python
"""Which launches an ICP call makes.  tests/golden/icp_routes.json lists calls on each side of every decision of the
strip-sweep launcher's plan (sfe_icp_sweep_plan.h) and, next to each, the route of every job (sfe_icp_last_routes) and
the launches a kernel trace showed for it.

  rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/icp_routes.py run [ROUTES.json]
      makes every call of the list once through the C ABI (sfe_icp_compute_jobs_chain_ext, with sfe_tune,
      sfe_icp_set_tuning and sfe_icp_get_profile as the call asks), on synthetic clouds; SONARFE_LIB picks the library.
      A 1 x 1 sfe_cfar_f32 call after each one marks in the trace where it ends.  The routes and the CU count go to
      ROUTES.json.
  python tools/icp_routes.py show DIR/t_kernel_trace.csv                 the launches per call, as text
  python tools/icp_routes.py record DIR/t_kernel_trace.csv ROUTES.json   write both into the fixture
  python tools/icp_routes.py check DIR/t_kernel_trace.csv [ROUTES.json]  compare with the fixture; exit status 1 on a
                                                                         difference

A call: `jobs` = groups of [source points, target points, count]: one cloud pair per group, `count` jobs on it (they
share the target's preparation), each with its own guess; `params` over icp_config.shipped_params(); `tune` (sfe_tune
knobs), `variant` (sfe_icp_set_tuning), `prof` (the counted profile on), `ox` (sfe_icp_outliers fields).  A launch is
recorded as {kernel, targs, workgroups, wg_size, lds}: the kernel's name and template arguments as the trace demangles
them, the grid in workgroups, and the LDS bytes of the dispatch as the trace reports them.  Routes are recorded as runs
[[route, jobs], ...].  make_call() is also what tests/test_gpu_icp_routes.py runs."""
import csv
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "icp_routes.json")
MARK = "cfar_f32_naive"


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def load_calls():
    return load_fixture()["calls"]


def clouds_of(call):
    """-> (src_all, tgt_all, jobs4, guesses9) of the call: scan pairs of sonar_slam_amd.synth, every guess perturbed"""
    from sonar_slam_amd import synth
    rng = np.random.default_rng(sum(map(ord, call["name"])))
    srcs, tgts, jobs, gs = [], [], [], []
    so = to = 0
    for k, (n_src, n_tgt, count) in enumerate(call["jobs"]):
        src, tgt, guess, _ = synth.scan_pair(seed=7000 + k, n_src=n_src, n_tgt=n_tgt)
        srcs.append(src)
        tgts.append(tgt)
        for _ in range(count):
            jobs.append((so, n_src, to, n_tgt))
            gs.append((guess.astype(np.float64) @ synth.pose_matrix(*rng.normal(0, [0.05, 0.05, 0.005]))).astype(np.float32))
        so += n_src
        to += n_tgt
    return (np.ascontiguousarray(np.concatenate(srcs), np.float32), np.ascontiguousarray(np.concatenate(tgts), np.float32),
            np.ascontiguousarray(jobs, np.int32), np.ascontiguousarray(gs, np.float32).reshape(len(jobs), 9))


def make_call(ctx, call, clouds, **tune):
    """-> (T [n x 3 x 3], status, iterations, routes); `tune` goes over the call's own knobs"""
    from sonar_slam_amd import _lib, icp_config
    C = _lib.C
    src, tgt, jobs4, g9 = clouds
    n = len(jobs4)
    p = icp_config.shipped_params(**call["params"])
    ox = _lib.IcpOutliers(**call["ox"]) if call["ox"] else None
    T, status, iters = np.zeros((n, 9), np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    f32, i32 = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    ctx._check(ctx.lib.sfe_icp_set_tuning(ctx.handle, call["variant"]))
    ctx._check(ctx.lib.sfe_icp_get_profile(ctx.handle, call["prof"], None))
    try:
        with ctx.tuning(**dict(call["tune"], **tune)):
            ctx._check(ctx.lib.sfe_icp_compute_jobs_chain_ext(
                ctx.handle, C.byref(p), C.byref(ox) if ox else None, None, 0, None, 0, src.ctypes.data_as(f32), len(src),
                tgt.ctypes.data_as(f32), len(tgt), jobs4.ctypes.data_as(i32), g9.ctypes.data_as(f32), n,
                T.ctypes.data_as(f32), status.ctypes.data_as(i32), iters.ctypes.data_as(i32)))
            routes = ctx.icp_routes(n)
    finally:
        ctx.lib.sfe_icp_set_tuning(ctx.handle, 0)
        ctx.lib.sfe_icp_get_profile(ctx.handle, 0, None)
    return T.reshape(n, 3, 3), status, iters, routes


def runs_of(routes):
    out = []
    for r in routes:
        if out and out[-1][0] == int(r):
            out[-1][1] += 1
        else:
            out.append([int(r), 1])
    return out


def run(routes_json):
    sys.path.insert(0, ROOT)
    from sonar_slam_amd import _lib
    ctx = _lib.default_context()
    one = np.zeros((1, 1), np.float32)
    out = np.zeros((1, 1), np.uint8)
    got = {"n_cu": ctx.n_cu, "routes": {}}
    for call in load_calls():
        _, status, iters, routes = make_call(ctx, call, clouds_of(call))
        got["routes"][call["name"]] = runs_of(routes)
        print("%-24s routes %s status %s iterations %d..%d" % (call["name"], got["routes"][call["name"]],
                                                               sorted(set(status.tolist())), iters.min(), iters.max()), flush=True)
        ctx._check(ctx.lib.sfe_cfar_f32(ctx.handle, one.ctypes.data_as(_lib.C.POINTER(_lib.C.c_float)), 1, 1, 0, 1, 0, 0,
                                        1.0, out.ctypes.data_as(_lib.C.POINTER(_lib.C.c_uint8)), None))
    if routes_json:
        with open(routes_json, "w") as f:
            json.dump(got, f)


def launches(trace_csv):
    """the trace's ICP launches per call of the list, in the order they ran"""
    with open(trace_csv, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    per_call, cur = [], []
    for r in rows:
        m = re.match(r"(?:void )?(\w+)(?:<(.*)>)?(?:\(|$)", r["Kernel_Name"])
        name = m.group(1) if m else r["Kernel_Name"]
        if name == MARK:
            per_call.append(cur)
            cur = []
        elif name.startswith("icp_"):
            wg = int(r["Workgroup_Size_X"])
            cur.append({"kernel": name, "targs": (m.group(2) or "").replace(" ", ""),
                        "workgroups": int(r["Grid_Size_X"]) // wg * int(r["Grid_Size_Y"]), "wg_size": wg,
                        "lds": int(r["LDS_Block_Size"])})
    calls = load_calls()
    assert len(per_call) == len(calls) and not cur, (len(per_call), len(calls), cur)
    return [(c, l) for c, l in zip(calls, per_call)]


def text(lau):
    if lau is None:
        return str(lau)
    return " + ".join("%s<%s> %d x %d lds %d" % (k["kernel"], k["targs"], k["workgroups"], k["wg_size"], k["lds"])
                      for k in lau)


def main():
    if len(sys.argv) < 2 or sys.argv[1] == "run":
        return run(sys.argv[2] if len(sys.argv) > 2 else None)
    got = launches(sys.argv[2])
    seen = None
    if len(sys.argv) > 3:
        with open(sys.argv[3]) as f:
            seen = json.load(f)
    if sys.argv[1] == "show":
        for c, lau in got:
            print("%-24s %s" % (c["name"], text(lau)))
    elif sys.argv[1] == "record":
        about = load_fixture()["about"]
        with open(FIXTURE, "w") as f:
            f.write('{"about": %s,\n "n_cu": %d,\n "calls": [\n' % (json.dumps(about), seen["n_cu"]))
            f.write(",\n".join("  " + json.dumps(dict(c, routes=seen["routes"][c["name"]], expect=lau)) for c, lau in got))
            f.write("\n]}\n")
    elif sys.argv[1] == "check":
        bad = [(c["name"], text(c.get("expect")), text(lau)) for c, lau in got if c.get("expect") != lau]
        for b in bad:
            print("%s: the fixture has %s, the trace %s" % b)
        if seen:
            if seen["n_cu"] != load_fixture().get("n_cu"):
                bad.append(("n_cu",))
                print("n_cu: the fixture has %s, the device %s" % (load_fixture().get("n_cu"), seen["n_cu"]))
            for c, _ in got:
                if seen["routes"][c["name"]] != c.get("routes"):
                    bad.append((c["name"],))
                    print("%s: the fixture has the routes %s, the call %s" % (c["name"], c.get("routes"), seen["routes"][c["name"]]))
        print("icp_routes: %d calls, %d differ" % (len(got), len(bad)))
        return 1 if bad else 0
    else:
        sys.exit(__doc__)


if __name__ == "__main__":
    sys.exit(main())
