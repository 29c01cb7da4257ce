"""The plan of an ICP call (sonar_slam_amd/csrc/sfe_icp_sweep_plan.h: the class of every job, the sizes that follow, the
build of every launch, the tables' layout and the order of the launches) is plain C++ without a HIP call.
tests/host/icp_plan_check.cpp runs it over a grid of job lists, chains, tuning values, flags and CU counts and checks the
invariants the executor and the kernels rely on; given the calls of tests/golden/icp_routes.json it also checks that
every call gets the routes, and launch by launch the kernel, the template arguments and the workgroups, that
sfe_icp_last_routes and the kernel trace of the commit before the header showed (tools/icp_routes.py wrote them there).
Here it is built with the host compiler and run on the CPU; the build line with the address and undefined-behaviour
sanitizers, for whoever changes the rules, is at the top of the .cpp file.  The GPU side: tests/test_gpu_icp_routes.py."""
import json
import os
import re
import subprocess

from sonar_slam_amd import icp_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("sw_tiers", "sw_tiny", "sw_multi", "sw_multi_g", "sw_multi_min_src", "sw_multi_share_min", "sw_strip_pts", "sw_rec")


def _tuning_defaults():
    """the shipped values of the knobs the plan reads (sfe_tuning, sfe_internal.h)"""
    with open(os.path.join(ROOT, "sonar_slam_amd", "csrc", "sfe_internal.h")) as f:
        found = dict(re.findall(r"^\s*int (sw_\w+) = (\d+);", f.read(), re.M))
    assert set(KNOBS) <= set(found)
    return {k: int(found[k]) for k in KNOBS}


def _lines(fixture):
    for c in fixture["calls"]:
        assert set(c["tune"]) <= set(KNOBS), c["name"]
        t = dict(_tuning_defaults(), **c["tune"])
        p = icp_config.shipped_params(**c["params"])
        ox = c["ox"] or {}
        line = [c["name"], fixture["n_cu"], p.minimizer, p.max_iter, p.use_diff_checker, p.normals_knn]
        line += [t[k] for k in KNOBS]
        line += [c["variant"], c["prof"], int(bool(ox.get("use_min_dist") or ox.get("use_median") or ox.get("use_bound")))]
        line += [len(c["jobs"])] + [v for g in c["jobs"] for v in g]
        line += [len(c["routes"])] + [v for r in c["routes"] for v in r]
        line += [len(c["expect"])]
        for e in c["expect"]:
            line += [e["kernel"], e["targs"], e["workgroups"], e["wg_size"], e["lds"]]
        yield " ".join(str(v) for v in line)


def test_icp_plan_check(tmp_path):
    with open(os.path.join(ROOT, "tests", "golden", "icp_routes.json")) as f:
        fixture = json.load(f)
    listing = tmp_path / "calls.txt"
    listing.write_text("\n".join(_lines(fixture)) + "\n")
    exe = str(tmp_path / "icp_plan_check")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                    os.path.join(ROOT, "tests", "host", "icp_plan_check.cpp"), "-o", exe], check=True, timeout=120)
    r = subprocess.run([exe, str(listing)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120,
                       universal_newlines=True)
    assert r.returncode == 0 and "icp_plan_check: ok" in r.stdout, r.stdout
    assert "%d calls of the fixture" % len(fixture["calls"]) in r.stdout, r.stdout
    assert "0 of 22 builds unreached" in r.stdout, r.stdout
