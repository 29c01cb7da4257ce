#!/usr/bin/env python
"""Which kernel a CFAR call takes.  tests/golden/cfar_routes.json lists calls on each side of every decision of the CFAR
dispatch (sfe_cfar_route.h) and, next to each, the launches a kernel trace showed for it.

  rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/cfar_routes.py run
      makes every call of the list once through the C ABI (sfe_cfar_u8_batch_dev / sfe_cfar_u8_bits_batch_dev, with
      sfe_cfar_set_tuning and sfe_tune as the call asks), on random images; SONARFE_LIB picks the library.  A 1 x 1
      sfe_cfar_f32 call after each one marks in the trace where it ends.
  python tools/cfar_routes.py show DIR/t_kernel_trace.csv      the launches per call, as text
  python tools/cfar_routes.py record DIR/t_kernel_trace.csv    write them into the fixture (`expect`)
  python tools/cfar_routes.py check DIR/t_kernel_trace.csv     compare them with the fixture; exit status 1 on a difference

A launch is recorded as {kernel, targs, workgroups, wg_size, lds}: the kernel's name and template arguments as the trace
demangles them, the grid in workgroups, and the LDS bytes of the dispatch (static + dynamic, as the trace reports them).
A call that is refused records "refused" and launches nothing.  make_call() is also what tests/test_gpu_cfar_routes.py
runs."""
import csv
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "cfar_routes.json")
MARK = "cfar_f32_naive"


def load_calls():
    with open(FIXTURE) as f:
        return json.load(f)["calls"]


def frames_of(call):
    """uniform random uint8 frames, the last one all 255"""
    rng = np.random.default_rng(sum(map(ord, call["name"])))
    fr = rng.integers(0, 256, (call["frames"], call["rows"], call["cols"]), dtype=np.uint8)
    fr[-1] = 255
    return fr


def make_call(ctx, call, frames):
    """-> (rc, masks, threshold maps or None); buffers are offset inside larger allocations as the call asks"""
    from sonar_slam_amd import _lib
    C = _lib.C
    n, rows, cols = frames.shape
    px = rows * cols
    bits = call["entry"] == "bits"
    wpf = (px + 31) // 32 + 1
    out_bytes = n * wpf * 4 if bits else n * px
    d_img, d_out = ctx.alloc(n * px + 16), ctx.alloc(out_bytes + 16)
    d_thr = ctx.alloc(n * px * 4 + 16) if call["thr"] else None
    at = lambda buf, off: C.c_void_p(buf.ptr.value + off)  # noqa: E731
    prev = {}
    try:
        d_img.upload(frames, offset=call["off_img"])
        d_out.upload(np.full(out_bytes, 0xA5, np.uint8), offset=call["off_out"])  # every byte must be written by the call
        ctx._check(ctx.lib.sfe_cfar_set_tuning(ctx.handle, call["tile_rows"], call["variant"]))
        for name, v in call["tune"].items():
            prev[name] = ctx.tune(name, v)
        args = (ctx.handle, at(d_img, call["off_img"]), n, rows, cols, _lib.ALG[call["alg"]], call["T"], call["G"],
                call["k"], float(call["tau"]), call["gate"], at(d_out, call["off_out"]))
        if bits:
            rc = ctx.lib.sfe_cfar_u8_bits_batch_dev(*args)
        else:
            rc = ctx.lib.sfe_cfar_u8_batch_dev(*(args + (at(d_thr, call["off_thr"]) if d_thr else None,)))
        ctx.sync()
        if rc != 0:
            return rc, None, None
        thr = d_thr.download(np.float32, n * px, offset=call["off_thr"]).reshape(frames.shape) if d_thr else None
        if bits:
            w = d_out.download(np.uint32, n * wpf, offset=call["off_out"]).reshape(n, wpf)
            b = np.stack([np.unpackbits(r.view(np.uint8), bitorder="little") for r in w])
            assert not b[:, px:].any(), "pad bits set"
            return rc, b[:, :px].reshape(frames.shape), thr
        return rc, d_out.download(np.uint8, n * px, offset=call["off_out"]).reshape(frames.shape), thr
    finally:
        ctx.lib.sfe_cfar_set_tuning(ctx.handle, 0, 0)
        for name, v in prev.items():
            ctx.tune(name, v)
        for b in (d_img, d_out, d_thr):
            if b is not None:
                b.free()


def run():
    sys.path.insert(0, ROOT)
    from sonar_slam_amd import _lib
    ctx = _lib.default_context()
    one = np.zeros((1, 1), np.float32)
    out = np.zeros((1, 1), np.uint8)
    for call in load_calls():
        rc, _, _ = make_call(ctx, call, frames_of(call))
        print("%-28s rc %d" % (call["name"], rc), flush=True)
        ctx._check(ctx.lib.sfe_cfar_f32(ctx.handle, one.ctypes.data_as(_lib.C.POINTER(_lib.C.c_float)), 1, 1, 0, 1, 0, 0,
                                        1.0, out.ctypes.data_as(_lib.C.POINTER(_lib.C.c_uint8)), None))


def launches(trace_csv):
    """the trace's CFAR launches per call of the list, in the order they ran"""
    with open(trace_csv, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    per_call, cur = [], []
    for r in rows:
        m = re.match(r"(?:void )?(\w+)(?:<(.*)>)?(?:\(|$)", r["Kernel_Name"])
        name = m.group(1) if m else r["Kernel_Name"]
        if name == MARK:
            per_call.append(cur)
            cur = []
        elif name.startswith("cfar_") or name.startswith("mask_pack"):
            wg = int(r["Workgroup_Size_X"])
            cur.append({"kernel": name, "targs": (m.group(2) or "").replace(" ", ""),
                        "workgroups": int(r["Grid_Size_X"]) // wg, "wg_size": wg, "lds": int(r["LDS_Block_Size"])})
    calls = load_calls()
    assert len(per_call) == len(calls) and not cur, (len(per_call), len(calls), cur)
    return [(c, l if l else "refused") for c, l in zip(calls, per_call)]


def text(lau):
    if lau is None or lau == "refused":
        return str(lau)
    return " + ".join("%s<%s> %d x %d lds %d" % (k["kernel"], k["targs"], k["workgroups"], k["wg_size"], k["lds"])
                      for k in lau)


def main():
    if len(sys.argv) < 2 or sys.argv[1] == "run":
        return run()
    got = launches(sys.argv[2])
    if sys.argv[1] == "show":
        for c, lau in got:
            print("%-28s %s" % (c["name"], text(lau)))
    elif sys.argv[1] == "record":
        with open(FIXTURE) as f:
            about = json.load(f)["about"]
        with open(FIXTURE, "w") as f:
            f.write('{"about": %s,\n "calls": [\n' % json.dumps(about))
            f.write(",\n".join("  " + json.dumps(dict(c, expect=lau)) for c, lau in got))
            f.write("\n]}\n")
    elif sys.argv[1] == "check":
        bad = [(c["name"], text(c.get("expect")), text(lau)) for c, lau in got if c.get("expect") != lau]
        for b in bad:
            print("%s: the fixture has %s, the trace %s" % b)
        print("cfar_routes: %d calls, %d differ" % (len(got), len(bad)))
        return 1 if bad else 0
    else:
        sys.exit(__doc__)


if __name__ == "__main__":
    sys.exit(main())
