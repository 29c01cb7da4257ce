"""CPU: the 3-D keyframe store's rules and surface (sfe_store3.hip, ``store.CloudStore3``), without a device.

- The device's transform rule -- per output coordinate fl(fma(p2, Hi2, fma(p1, Hi1, fl(p0 * Hi0))) + Hi3), restated with
  correctly rounded fused operations in tests/store3_ref.py -- equals the reference's numpy expression
  ``points.dot(H[:3, :3].T) + H[:3, 3]`` on every input the GPU tests use.  If another BLAS rounds differently, it shows here.
- Clouds with z = 0 under a planar H reproduce the 2-D SFE_STORE_F32_POINTS rule (fl(fma(p1, r1, fl(p0 * r0)) + t)) in x, y.
- The ABI symbols and signatures exist; the C entry points return an error for a NULL context before touching a device.
- ``CloudStore3.icp`` raises the refusals of ``pcl.ICP._chain3``.
- tests/host/store3_slots_check.cpp (the slot and pool arithmetic of sfe_store3_slots.h) builds and passes, plain and under
  the address and undefined-behaviour sanitizers.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from sonar_slam_amd import _lib as L
from sonar_slam_amd import icp_config, store

import icp3_cases as C
import store3_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_fma_chain_equals_numpy_on_every_gpu_input():
    n_floats = 0
    for pts, H in R.fixed_inputs():
        a, b = R.transform(pts, H), R.transform_fma(pts, H)
        assert a.dtype == np.float32 and a.shape == b.shape == (len(pts), 3)
        assert np.array_equal(a, b, equal_nan=True), (len(pts), int((a != b).sum()))
        n_floats += a.size
    assert n_floats > 100000


def test_the_plain_rounded_chain_is_another_rule():
    """what the fused rule is held against: every product and sum rounded differs in a good part of the floats"""
    pts, H = R.cloud(1, 4097), R.motion(2)
    plain = np.zeros_like(pts)
    for i in range(3):
        acc = (pts[:, 0] * H[i, 0]).astype(f32)
        acc = (acc + (pts[:, 1] * H[i, 1]).astype(f32)).astype(f32)
        acc = (acc + (pts[:, 2] * H[i, 2]).astype(f32)).astype(f32)
        plain[:, i] = (acc + H[i, 3]).astype(f32)
    assert (plain != R.transform(pts, H)).mean() > 0.05


def test_planar_input_reproduces_the_2d_f32_rule():
    pts = R.cloud(4, 3001)
    pts[:, 2] = 0
    th, tx, ty = 0.7, 31.5, -17.25
    H = np.asarray(C.planar_motion(tx, ty, th), f32)
    got = R.transform_fma(pts, H)
    # the F32_POINTS rule of the 2-D store (sfe_store.hip): fl(fma(p1, r1, fl(p0 * r0)) + t)
    for i in range(2):
        acc = (pts[:, 0] * H[i, 0]).astype(f32)
        want = (R._fma32(pts[:, 1], H[i, 1], acc) + H[i, 3]).astype(f32)
        assert np.array_equal(got[:, i], want)
    assert np.array_equal(got[:, 2], np.zeros(len(pts), f32))
    assert np.array_equal(got, R.transform(pts, H))


def test_symbols_and_signatures():
    names = ["sfe_cloud_store3_create", "sfe_cloud_store3_destroy", "sfe_cloud_store3_count", "sfe_cloud_store3_put",
             "sfe_cloud_store3_meta", "sfe_cloud_store3_read", "sfe_cloud_store3_truncate", "sfe_cloud_store3_get_points",
             "sfe_icp3_store_compute", "sfe_cloud_store3_overlap"]
    hdr = open(os.path.join(ROOT, "include", "sonarfe.h")).read()
    lib = L.load_library()
    for name in names:
        assert name in L.SIGNATURES and hasattr(lib, name) and name + "(" in hdr, name
    assert "typedef struct sfe_cloud_store3 sfe_cloud_store3;" in hdr
    assert ("int sfe_cloud_store3_get_points(sfe_ctx *ctx, sfe_cloud_store3 *s, const int32_t *handles, const float *H12, "
            "int n_jobs, int m,") in hdr
    assert len(L.SIGNATURES["sfe_cloud_store3_get_points"][1]) == 9
    assert len(L.SIGNATURES["sfe_icp3_store_compute"][1]) == 9
    assert len(L.SIGNATURES["sfe_cloud_store3_overlap"][1]) == 7
    mk = open(os.path.join(ROOT, "sonar_slam_amd", "csrc", "Makefile")).read()
    assert "sfe_store3.hip" in mk


def test_null_context_is_an_error_before_any_device_call():
    lib = L.load_library()
    out = ctypes.c_void_p()
    h = ctypes.c_int32(7)
    n = ctypes.c_int(7)
    assert lib.sfe_cloud_store3_create(None, 1000, 10, ctypes.byref(out)) < 0 and not out.value
    assert lib.sfe_cloud_store3_put(None, None, 0, None, 0, ctypes.byref(h)) < 0 and h.value == 7
    assert lib.sfe_cloud_store3_meta(None, None, 0, 0, None, None, None) < 0
    assert lib.sfe_cloud_store3_read(None, None, 0, None, 0, ctypes.byref(n)) < 0 and n.value == 7
    assert lib.sfe_cloud_store3_truncate(None, None, 0) < 0
    assert lib.sfe_cloud_store3_get_points(None, None, None, None, 0, 1, 0.5, None, None) < 0
    assert lib.sfe_icp3_store_compute(None, None, None, None, None, 0, None, None, None) < 0
    assert lib.sfe_cloud_store3_overlap(None, None, None, None, 0, 1.0, None) < 0
    assert lib.sfe_cloud_store3_count(None) == 0
    lib.sfe_cloud_store3_destroy(None)


class _NoDevice(object):
    """a context that fails the test if a refused call reaches the library"""
    def __getattr__(self, name):
        raise AssertionError("the call reached the device context (%s)" % name)


def test_icp_raises_the_chain3_refusals():
    s = store.CloudStore3.__new__(store.CloudStore3)         # no device: the refusals come before any library call
    s.ctx, s.handle = _NoDevice(), None
    pairs, g = np.array([[0, 1]], np.int32), np.eye(4, dtype=f32)[None]
    stage = L.IcpDpf(kind=L.DPF_MAX_DIST, dim=-1, remove_inside=0)
    stage.f[0] = 20.0
    chains = [(icp_config.IcpChain(icp_config.shipped_params(), reading=[stage]), "data-point filters"),
              (icp_config.IcpChain(icp_config.shipped_params(), reference=[stage]), "data-point filters"),
              (icp_config.IcpChain(icp_config.shipped_params(), outliers=L.IcpOutliers(use_median=1, median_factor=3.0)),
               "MedianDist"),
              (icp_config.IcpChain(icp_config.shipped_params(minimizer=1)), "PointToPlane"),
              (icp_config.shipped_params(minimizer=1), "PointToPlane")]
    for chain, what in chains:
        with pytest.raises(NotImplementedError, match=what) as e:
            s.icp(pairs, g, chain)
        assert "CloudStore3.icp" in str(e.value)
    with pytest.raises(TypeError, match="IcpParams"):
        s.icp(pairs, g, None)
    with pytest.raises(TypeError, match="4 x 4"):
        store.pose_H12(np.eye(3))
    assert np.array_equal(store.pose_H12(np.arange(16).reshape(4, 4)), np.arange(12, dtype=f32))


def _build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + extra +
                   [os.path.join(ROOT, "tests", "host", "store3_slots_check.cpp"), "-o", exe], check=True, timeout=180)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, universal_newlines=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("store3_slots_check: ok"), r.stdout[-2000:]


def test_slots_check_builds_and_passes(tmp_path):
    _build(tmp_path, "store3_slots_check", [])


def test_slots_check_under_sanitizers(tmp_path):
    """the same program with the address and undefined-behaviour sanitizers, as a stand-alone program"""
    _build(tmp_path, "store3_slots_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
