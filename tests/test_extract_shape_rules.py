"""The launch shape of extract_gather_kernel (sonar_slam_amd/csrc/sfe_extract_shape.h: workgroups per frame, piece size,
and the index arithmetic from a workgroup's running word to a word of the frame's bit stream) is plain C++ without a HIP
call, shared by ExtractCall and the kernel.  tests/host/extract_shape_check.cpp runs it for every chunk size 1 .. 1024,
with and without the record path, over frames of 1 to 2^27 - 32 stream words: bounds of slices and piece_shift (the
record layout and s_rp[66] of extract_merge_expand_kernel hang on them), every stream word visited exactly once, no int
overflow, the per-frame rotation a permutation.  Here it is built with the host compiler that the oracle's Makefile uses
and run on the CPU; the build line with the address and undefined-behaviour sanitizers, for whoever changes the rules,
is at the top of the .cpp file.  The GPU side of the same quantities: tests/test_gpu_extract_batches.py."""
import importlib.util
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "extract_shape_check")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                    os.path.join(ROOT, "tests", "host", "extract_shape_check.cpp"), "-o", exe], check=True, timeout=120)
    return exe


def test_extract_shape_check(tmp_path):
    r = subprocess.run([_build(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120,
                       universal_newlines=True)
    assert r.returncode == 0 and "extract_shape_check: ok" in r.stdout, r.stdout


def test_the_tools_copy_of_the_slices_rule_follows_gather_shape(tmp_path):
    """tools/extract_records_stats.py reads scratch slot 62 with a stride of slices + 1 and so repeats the slices rule in
    Python: equal to gather_shape for every chunk size, with and without the record path, on the bench geometry (16384
    stream words) and on frames small enough for the cap by stream words (192, 65, 1)"""
    spec = importlib.util.spec_from_file_location("extract_records_stats",
                                                  os.path.join(ROOT, "tools", "extract_records_stats.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    exe = _build(tmp_path)
    for nwords in (16384, 4096, 192, 65, 1):
        r = subprocess.run([exe, "--table", str(nwords)], stdout=subprocess.PIPE, timeout=120, universal_newlines=True,
                           check=True)
        rows = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
        assert len(rows) == 2048
        for records, nf, slices, _ in rows:
            assert tool.gather_slices(nwords, bool(records), nf) == slices, (nwords, records, nf)
