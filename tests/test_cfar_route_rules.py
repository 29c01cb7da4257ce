"""The route of a CFAR call (sonar_slam_amd/csrc/sfe_cfar_route.h: which kernel, which template instance, the launch shape
and the decision tables) is plain C++ without a HIP call.  tests/host/cfar_route_check.cpp runs it over a grid of shapes,
algorithms, windows, output kinds, tuning variants and alignments and checks the invariants the kernels rely on; given the
calls of tests/golden/cfar_routes.json it also checks that every call takes the kernel, the instance and the number of
workgroups that the kernel trace of the commit before the header showed (tools/cfar_routes.py wrote them there).  Here it
is built with the host compiler and run on the CPU; the build line with the address and undefined-behaviour sanitizers,
for whoever changes the rules, is at the top of the .cpp file.  The GPU side: tests/test_gpu_cfar_routes.py."""
import json
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALG = {"CA": 0, "SOCA": 1, "GOCA": 2, "OS": 3}


def _align(offset):
    """cfar_align_of an address `offset` bytes into a device allocation"""
    return next(a for a in (16, 8, 4, 2, 1) if offset % a == 0)


def _tuning_defaults():
    """the shipped cfar_os_* values (sfe_tuning, sfe_internal.h)"""
    with open(os.path.join(ROOT, "sonar_slam_amd", "csrc", "sfe_internal.h")) as f:
        found = dict(re.findall(r"^\s*int (cfar_os_\w+) = (\d+);", f.read(), re.M))
    assert set(found) == {"cfar_os_gated", "cfar_os_gated_min", "cfar_os_pref", "cfar_os_pref_x"}
    return {k: int(v) for k, v in found.items()}


def _lines(calls):
    for c in calls:
        t = dict(_tuning_defaults(), **c["tune"])
        head = [c["name"], int(c["entry"] == "bits"), c["frames"], c["rows"], c["cols"], ALG[c["alg"]], c["T"], c["G"], c["k"],
                repr(float(c["tau"])), c["gate"], int(c["thr"]), _align(c["off_img"]), _align(c["off_out"]),
                _align(c["off_thr"]) if c["thr"] else 0, c["variant"], c["tile_rows"], t["cfar_os_gated"],
                t["cfar_os_gated_min"], t["cfar_os_pref"], t["cfar_os_pref_x"]]
        e = c["expect"]
        if e == "refused":
            tail = ["refused"]
        else:
            packed = len(e) == 2
            assert len(e) == 1 or (packed and c["entry"] == "bits" and e[1]["kernel"] == "mask_pack_kernel"), c["name"]
            tail = [e[0]["kernel"], e[0]["targs"] or "-", e[0]["workgroups"], e[0]["wg_size"], int(packed)]
        yield " ".join(str(v) for v in head + tail)


def test_cfar_route_check(tmp_path):
    with open(os.path.join(ROOT, "tests", "golden", "cfar_routes.json")) as f:
        calls = json.load(f)["calls"]
    listing = tmp_path / "calls.txt"
    listing.write_text("\n".join(_lines(calls)) + "\n")
    exe = str(tmp_path / "cfar_route_check")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                    os.path.join(ROOT, "tests", "host", "cfar_route_check.cpp"), "-o", exe], check=True, timeout=120)
    r = subprocess.run([exe, str(listing)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120,
                       universal_newlines=True)
    assert r.returncode == 0 and "cfar_route_check: ok" in r.stdout, r.stdout
    assert "%d calls of the fixture" % len(calls) in r.stdout, r.stdout
