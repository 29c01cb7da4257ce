#!/usr/bin/env python
"""HIP-event time of the resident cloud filters on the bench frames and the phase stamps of cf_downsample_radix_kernel.

    python tools/filter_phases.py [frames] [repeats]

Times run_filter like tools/extract_times.py (SONARFE_LIB picks the library), then -- where the library has
sfe_cf_get_profile -- runs the stamped build of the downsample kernel and prints what workgroup 0 (frame 0) spent in
each phase, in clock64() ticks: once for the two-kernel route (downsampled clouds to HBM, cf_radius_filter_kernel on
every frame) and once for the shipped route with the outlier filter in the kernel's tail."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import bench  # noqa: E402
from sonar_slam_amd import _lib, icp_config, synth  # noqa: E402
from sonar_slam_amd.CFAR import CFAR  # noqa: E402
from sonar_slam_amd.feature_extraction import FeatureExtraction, SonarPing, oculus_bearings  # noqa: E402
from sonar_slam_amd.pipeline import KeyframeBatch  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
PHASES = ["keys", "sort pass 0", "sort pass 1", "sort pass 2", "sort pass 3", "leaf scan + starts", "point gather", "medoids",
          "radius filter / end"]

ctx = _lib.default_context()
det = CFAR(40, 10, 0.1, 10)
fe = FeatureExtraction(ctx)
fe.Ntc, fe.Ngc, fe.Pfa, fe.rank, fe.alg, fe.threshold = 40, 10, 0.1, 10, "SOCA", 65
fe.configure()
base = [synth.sonar_frame(seed=s) for s in range(min(B, 32))]          # bench.make_inputs(0, B)'s frames
frames = np.stack([base[j % len(base)] for j in range(B)])
fe.generate_map_xy(SonarPing(frames[0], oculus_bearings(bench.COLS), 30.0 / bench.ROWS))
kb = KeyframeBatch(ctx, fe.geometry, det.params["SOCA"], "SOCA", 65, icp_config.shipped_params(), B, max_points=32768)   # the bench's capacity
kb.upload_frames(frames)
kb.run_cfar()
kb.run_extract()


def timed(fn, reps):
    fn()
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


for r in range(REPS):
    print("filter %.3f ms / %d frames (run %d)" % (timed(kb.run_filter, 5), B, r))
res = kb.results()
print("frame 0: %d points, %d after the filters; points/frame %.0f, after the filters %.0f"
      % (res["counts"][0], res["cloud_counts"][0], res["counts"].mean(), res["cloud_counts"].mean()))

get_profile = getattr(ctx.lib, "sfe_cf_get_profile", None)
if get_profile is None:
    print("this library has no sfe_cf_get_profile: no phase stamps")
    sys.exit(0)
get_profile.restype = C.c_int
get_profile.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_longlong)]
stamps = (C.c_longlong * 16)()
for mode, name in ((2, "two-kernel route"), (1, "tail in the kernel")):
    for r in range(REPS):
        ctx._check(get_profile(ctx.handle, mode, None))
        kb.run_filter()
        ctx._check(get_profile(ctx.handle, 0, stamps))
        t = list(stamps)[:10]
        last, parts = t[0], []
        for k in range(1, 10):
            if t[k]:
                parts.append("%s %d" % (PHASES[k - 1], t[k] - last))
                last = t[k]
        print("stamps, %s (run %d): total %d ticks: %s" % (name, r, last - t[0], "; ".join(parts)))
