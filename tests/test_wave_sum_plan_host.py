"""The plan of the transposed wave reduction (sonar_slam_amd/csrc/sfe_wave_sum_plan.h: per level each lane's partner, the
accumulators it keeps and hands over, the lane that ends up with each row total, the row order) is plain C++ without a HIP
call, shared by wave_sum_n (sfe_icp_common.h) and tests/host/wave_sum_plan_check.cpp.  The program runs the plan on 64
simulated lanes of doubles -- random values, 30 binades with heavy cancellation, signed zeros, single non-zero lanes, one
row alone -- and compares all nine totals bit for bit with a literal restatement of wave_sum; on the cancelling inputs it
also shows that another row association and another butterfly do not give those bits.  Here it is built with the host
compiler that the oracle's Makefile uses and run on the CPU; the build line with the address and undefined-behaviour
sanitizers, for whoever changes the plan, is at the top of the .cpp file.  The GPU side: tests/test_gpu_icp_sums_reduce.py."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wave_sum_plan_check(tmp_path):
    exe = str(tmp_path / "wave_sum_plan_check")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                    os.path.join(ROOT, "tests", "host", "wave_sum_plan_check.cpp"), "-o", exe], check=True, timeout=120)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, universal_newlines=True)
    assert r.returncode == 0 and "wave_sum_plan_check: ok" in r.stdout, r.stdout
    m = re.search(r"of (\d+) cancelling inputs (\d+) tell the row association apart, (\d+) the butterfly", r.stdout)
    assert m and int(m.group(2)) > 0 and int(m.group(3)) > 0, r.stdout
