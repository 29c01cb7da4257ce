"""The generation rules of the strip-sweep ICP launcher (sonar_slam_amd/csrc/sfe_icp_gen.h: which copy of the
prepared-target scratch a batch uses, which earlier loop kernels its preparation waits for) are plain C++ without a HIP
call.  tests/host/icp_gen_check.cpp runs them over every sequence of up to 9 batches (up to 6 with launches that fail
half-way) against a model of the two streams.  Here it is built with the host compiler that the oracle's Makefile uses
and run on the CPU; the build line with the address and undefined-behaviour sanitizers, for whoever changes the rules,
is at the top of the .cpp file."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_icp_gen_check(tmp_path):
    exe = str(tmp_path / "icp_gen_check")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                    os.path.join(ROOT, "tests", "host", "icp_gen_check.cpp"), "-o", exe], check=True, timeout=120)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, universal_newlines=True)
    assert r.returncode == 0 and "icp_gen_check: ok" in r.stdout, r.stdout
