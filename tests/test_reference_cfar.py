"""CFAR pinned to the reference implementation ITSELF: bruce_slam/src/bruce_slam/cpp/cfar.cpp is
compiled unmodified, from the reference tree, against a 40-line stand-in for the two Eigen types it
uses (oracle/ref_shim, recipe oracle/Makefile) into oracle/_ref/libcfar_ref.so.
The oracle's C restatement and the HIP kernels must reproduce it bit for bit.

Every output of the reference on these cases is recorded in golden/cfar_ref_digest.json (SHA-256 of the
array's bytes, with dtype and shape; written by golden/make_golden.py from the compiled library), so the
tests hold on any checkout; where oracle/_ref is built they compare against the live library as well."""
import hashlib
import json
import os

import numpy as np
import pytest

import oracle
from sonar_slam_amd import synth
from sonar_slam_amd.CFAR import CFAR

DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cfar_ref_digest.json")
ALGS = ["CA", "SOCA", "GOCA", "OS"]


def _params(alg, det):
    p = det.params[alg]
    return (p[0], p[1], p[3], p[2]) if alg == "OS" else (p[0], p[1], p[2], 0)   # train_hs, guard_hs, tau, k


def digest(a):
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        a = a + a.dtype.type(0)      # -0.0 -> +0.0: equal digests exactly where np.array_equal holds
    return "%s %s %s" % (a.dtype.str, "x".join(str(n) for n in a.shape), hashlib.sha256(a.tobytes()).hexdigest())


def host_cases(alg):
    """-> [(key, image, train_hs, guard_hs, tau, k, want_threshold)] of the host test, random images drawn in this order"""
    det = CFAR(40, 10, 0.1, 10)                       # feature.yaml:3-7
    th, gh, tau, k = _params(alg, det)
    rng = np.random.default_rng(11)
    frames = [synth.sonar_frame(seed=3, rows=300, cols=96, n_blobs=10),
              rng.integers(0, 256, (120, 40), dtype=np.uint8),
              np.full((90, 17), 255, np.uint8), np.zeros((64, 9), np.uint8),
              rng.integers(0, 256, (50, 12), dtype=np.uint8),      # shorter than the window: all-zero mask
              (rng.random((140, 33)) * 300).astype(np.float32)]    # non-uint8 caller
    cases = []
    for i, img in enumerate(frames):
        cases.append(("host_%s_frame%d_thr" % (alg, i), img, th, gh, tau, k, True))
        cases.append(("host_%s_frame%d" % (alg, i), img, th, gh, tau, k, False))
    # other windows / taus
    for (t, g, ta) in ((4, 1, 1.3), (10, 0, 2.0), (7, 3, 0.9)):
        img = rng.integers(0, 256, (80, 20), dtype=np.uint8)
        cases.append(("host_%s_window%d_%d_%g" % (alg, t, g, ta), img, t, g, ta, min(k, 2 * t - 1), False))
    return cases


def full_size_cases(alg):
    """the BASELINE frame shape: 1024 x 512"""
    th, gh, tau, k = _params(alg, CFAR(40, 10, 0.1, 10))
    img = synth.sonar_frame(seed=17)
    return [("full_%s" % alg, img, th, gh, tau, k, False), ("full_%s_thr" % alg, img, th, gh, tau, k, True)]


def reference_digests(cases):
    """what the compiled reference returns on `cases`, as digests -> {key: [digest, ...]} (make_golden.py)"""
    out = {}
    for key, img, th, gh, tau, k, thr in cases:
        alg = key.split("_")[1]
        got = oracle.ref_cfar(img, alg, th, gh, tau, k, want_threshold=thr)
        out[key] = [digest(a) for a in (got if thr else (got,))]
    return out


def expect_reference(key, img, alg, th, gh, tau, k, thr, got):
    """`got` (mask, or (mask, threshold map) with thr) is what the reference returned on this case"""
    got = tuple(np.asarray(a) for a in (got if thr else (got,)))
    assert [digest(a) for a in got] == json.load(open(DIGESTS))[key], key
    if oracle.have_ref_cfar():
        want = oracle.ref_cfar(img, alg, th, gh, tau, k, want_threshold=thr)
        for a, b in zip(got, want if thr else (want,)):
            assert np.array_equal(a, b), key


@pytest.mark.parametrize("alg", ALGS)
def test_oracle_restatement_equals_compiled_reference(alg):
    for key, img, th, gh, tau, k, thr in host_cases(alg):
        expect_reference(key, img, alg, th, gh, tau, k, thr, oracle.cfar(img, alg, th, gh, tau, k, want_threshold=thr))


@pytest.mark.gpu
@pytest.mark.parametrize("alg", ALGS)
def test_hip_cfar_equals_compiled_reference_full_size(alg):
    """the HIP kernels against the reference's own code on the BASELINE frame shape"""
    from sonar_slam_amd import cfar
    for key, img, th, gh, tau, k, thr in full_size_cases(alg):
        fn = getattr(cfar, alg.lower() + ("2" if thr else ""))
        got = fn(img, th, gh, k, tau) if alg == "OS" else fn(img, th, gh, tau)
        expect_reference(key, img, alg, th, gh, tau, k, thr, got)
