"""CPU: the keyed clouds of the 3-D keyframe store (sfe_store3.hip, ``store.CloudStore3``) without a device -- that every input
tests/test_gpu_store3_keys.py builds holds what it was built for, shown on the references alone (tests/store3_keys_ref.py):

- the range expression equals ``np.linalg.norm(axis=1)`` on float32 N x 3 input, bit for bit, and ``store.fov3_numpy`` equals
  the reference gate;
- the tie cases have equal float distances, inside one tile and across tile borders, with different keys at the tied indices;
- the on-the-bound cases are exactly on their bounds;
- coincident points of two clouds land in one leaf and the earlier cloud's key wins;
- the gate condition: on every gate input but the one built to sit on its bearing bound, every point / frame pair that passes
  the range test has | |bearing| - bound | > 1e-5 |bearing| + 1e-29 -- ten times the kernel's margin (1e-6 a + 1e-30), so the
  reference alone guarantees that the device decides every point (n_ambiguous == 0, which the GPU tests assert).  A condition
  on the inputs, not a tolerance on a result;
- the Python layer refuses bad arguments before any library call; header, ``SIGNATURES`` and exported symbols agree and every
  new entry point returns an error for a NULL context;
- tests/host/store3_keys_check.cpp (flags, bounds and the job table of sfe_store3_slots.h) builds and passes, plain and under
  the address and undefined-behaviour sanitizers.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from sonar_slam_amd import _lib as L
from sonar_slam_amd import store
from sonar_slam_amd.store import fov3_numpy  # noqa: F401  (the first new name: without the feature nothing here runs)

import pcl3_ref
import store3_keys_ref as K
import store3_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

NEW = ["sfe_cloud_store3_put_keys", "sfe_cloud_store3_keyed", "sfe_cloud_store3_get_points_keys", "sfe_cloud_store3_read_keys",
       "sfe_cloud_store3_fov_select", "sfe_cloud_store3_set_selection", "sfe_cloud_store3_compact_selected",
       "sfe_cloud_store3_match_keys"]


def _all_gates():
    yield from K.gate_inputs()
    p, _, H, rb, bb, _ = K.fov_on_the_bearing_bound()
    yield p, H, rb, bb


def test_range_expression_is_numpys_norm_and_fov3_numpy_is_the_reference_gate():
    n = 0
    for pts, Hinvs, rbs, bbs in _all_gates():
        for H, rb, bb in zip(Hinvs, rbs, bbs):
            local = R.transform_fma(pts, H)
            assert np.array_equal(local, R.transform(pts, H), equal_nan=True)
            with np.errstate(invalid="ignore", over="ignore"):
                want = np.linalg.norm(local, axis=1)
            got = K.range3(local)
            assert want.dtype == got.dtype == np.float32 and np.array_equal(got, want, equal_nan=True)
            assert np.array_equal(store.fov3_numpy(pts, H, rb, bb), K.fov_frame(pts, H, rb, bb))
            n += len(pts)
    assert n > 10000
    # a cloud where the order of the three additions shows: the sum is not the one of another association
    x = R.cloud(5, 4000)
    other = np.sqrt((x[:, 0] * x[:, 0] + (x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2]).astype(f32)).astype(f32))
    assert (other != K.range3(x)).any() and np.array_equal(K.range3(x), np.linalg.norm(x, axis=1))


def test_tie_cases_are_ties_with_different_keys():
    src, tgt, keys, max_dist, pairs = K.tie_case()
    assert len(tgt) == 2 * K.TILE + 3
    tiles = set()
    for s, (lo, hi) in enumerate(pairs):
        d = pcl3_ref.dist2(src[s], tgt)
        assert lo < hi and d[lo] == d[hi] == d.min() and (d == d.min()).sum() == 2
        assert d[lo] <= f32(max_dist) * f32(max_dist)
        assert keys[lo] != keys[hi]
        tiles.add((lo // K.TILE, hi // K.TILE))
    assert (0, 0) in tiles and (0, 1) in tiles and (0, 2) in tiles and (1, 2) in tiles     # inside a tile and across borders
    assert (K.TILE - 1, K.TILE) in pairs                                                  # the two sides of a border
    hist, ov = K.match_keys(src, R.EYE, tgt, keys, max_dist, 40)
    assert ov == len(pairs)
    for s, (lo, hi) in enumerate(pairs):
        assert hist[keys[lo]] == 1 and hist[keys[hi]] == 0


def test_bound_cases_are_exactly_on_their_bounds():
    # the radius: d2 == r2 and the next float above
    src, tgt, keys, max_dist, want, hist = K.radius_case()
    r2 = f32(max_dist) * f32(max_dist)
    assert pcl3_ref.dist2(src[0], tgt)[0] == r2 and pcl3_ref.dist2(src[6], tgt)[1] == r2
    assert pcl3_ref.dist2(src[-1], tgt)[0] == np.nextafter(r2, f32(1)) and pcl3_ref.dist2(src[1], tgt)[0] > r2
    got_hist, got = K.match_keys(src, R.EYE, tgt, keys, max_dist, 2)
    assert got == want and np.array_equal(got_hist, hist)
    # the range: exactly the bound, and the float below it
    pts, keys, Hinvs, rb, bb, sel, n_keys = K.fov_special()
    local = R.transform_fma(pts, Hinvs[0])
    assert np.array_equal(local[:6], pts[:6])
    rng = K.range3(local)
    assert float(rng[0]) == rb[0] and float(rng[1]) < rb[0] and rng[1] == np.nextafter(f32(rb[0]), f32(0))
    assert np.array_equal(K.fov(pts, Hinvs, rb, bb), sel)
    assert abs(np.arctan2(local[3, 1], local[3, 0])) == f32(np.pi) and np.arctan2(local[4, 1], local[4, 0]) == -f32(np.pi)
    assert (keys[sel == 1] >= n_keys).sum() == 2
    # the bearing: the double-precision bearing of the chosen point is the bound itself
    pts, keys, Hinvs, rb, bb, i = K.fov_on_the_bearing_bound()
    gaps, angles = K.fov_margins(pts[i:i + 1], Hinvs, rb, bb)
    assert len(gaps) == 1 and gaps[0] == 0.0
    gaps, angles = K.fov_margins(np.delete(pts, i, axis=0), Hinvs, rb, bb)
    assert np.all(gaps > 1e-5 * angles + 1e-29)          # every other point of that cloud is decided


def test_coincident_points_share_a_leaf_and_the_earlier_cloud_wins():
    clouds, Hs, keys, res = K.coincident_job()
    a, b = clouds
    cat = np.concatenate([R.transform_fma(c, H) for c, H in zip(clouds, Hs)])
    assert np.array_equal(cat[:len(a)], a) and np.array_equal(cat[len(a):len(a) + len(a)], a[::-1])
    info = {}
    pts, idx = pcl3_ref.downsample(cat, res, info)
    twin = {i: len(a) + (len(a) - 1 - i) for i in range(len(a))}
    leaf_of = {}
    for k, leaf in enumerate(info["leaves"]):
        for i in leaf:
            leaf_of[int(i)] = k
    assert all(leaf_of[i] == leaf_of[j] for i, j in twin.items())
    got_pts, got_keys = K.get_points_keys(clouds, Hs, keys, res)
    shared = idx < 2 * len(a)
    assert shared.sum() >= 100 and np.all(idx[shared] < len(a))          # the medoid is the earlier cloud's point ...
    assert np.all(got_keys[shared] == keys[0]) and np.all(got_keys[~shared] == keys[1]) and (~shared).sum() == 2


def test_gate_condition_holds_on_every_gate_input():
    n_pairs = 0
    for pts, Hinvs, rbs, bbs in K.gate_inputs():
        gaps, angles = K.fov_margins(pts, Hinvs, rbs, bbs)
        bad = ~(gaps > 1e-5 * angles + 1e-29)
        assert not bad.any(), (len(pts), gaps[bad], angles[bad])
        n_pairs += len(gaps)
    assert n_pairs > 3000


class _NoDevice(object):
    """a context that fails the test if a refused call reaches the library"""
    def __getattr__(self, name):
        raise AssertionError("the call reached the device context (%s)" % name)


def test_python_layer_refuses_bad_arguments_before_any_library_call():
    s = store.CloudStore3.__new__(store.CloudStore3)
    s.ctx, s.handle = _NoDevice(), None
    pts = np.zeros((4, 3), f32)
    E = np.eye(4, dtype=f32)
    with pytest.raises(ValueError, match="N x 3"):
        s.put_keys(np.zeros((4, 2), f32), [0, 1, 2, 3])
    with pytest.raises(ValueError, match="3 keys for 4 points"):
        s.put_keys(pts, [0, 1, 2])
    with pytest.raises(ValueError, match="integers in"):
        s.put_keys(pts, [0, 1, -2, 3])
    with pytest.raises(ValueError, match="integers in"):
        s.put_keys(pts, [0, 1, 2.5, 3])
    with pytest.raises(ValueError, match="integers in"):
        s.put_keys(pts, [0, 1, 2 ** 31, 3])
    with pytest.raises(ValueError, match="1 transform lists and 2 key lists"):
        s.get_points_keys([[0], [1]], [[E]], [[0], [1]], 0.1)
    with pytest.raises(ValueError, match="target 1 lists 2 handles but 1 transforms"):
        s.get_points_keys([[0], [1, 2]], [[E], [E]], [[0], [1, 2]], 0.1)
    with pytest.raises(ValueError, match="target 1: 1 keys for 2 handles"):
        s.get_points_keys([[0], [1, 2]], [[E], [E, E]], [[0], [1]], 0.1)
    with pytest.raises(ValueError, match="integers in"):
        s.get_points_keys([[0]], [[E]], [[-1]], 0.1)
    with pytest.raises(TypeError, match="4 x 4"):
        s.get_points_keys([[0]], [[np.eye(3)]], [[1]], 0.1)
    with pytest.raises(ValueError, match="2 handles but 1 frame lists"):
        s.fov_select([0, 1], [[E]], [[1.0], [1.0]], [[1.0], [1.0]], 4)
    with pytest.raises(ValueError, match="cloud 0 has 2 frames but 1 range bounds"):
        s.fov_select([0], [[E, E]], [[1.0]], [[1.0, 2.0]], 4)
    with pytest.raises(ValueError, match="n_keys"):
        s.fov_select([0], [[E]], [[1.0]], [[1.0]], -1)
    with pytest.raises(TypeError, match="4 x 4"):
        s.fov_select([0], [[np.eye(3)]], [[1.0]], [[1.0]], 4)
    with pytest.raises(ValueError, match="2 pairs but 1 transforms"):
        s.match_keys([[0, 1], [2, 3]], [E], 0.5, 4)
    with pytest.raises(ValueError, match="n_keys"):
        s.match_keys([[0, 1]], [E], 0.5, -1)
    with pytest.raises(TypeError, match="4 x 4"):
        s.match_keys([[0, 1]], [np.zeros((3, 4))], 0.5, 4)


def test_fov3_numpy_is_the_reference_expression():
    pts, _, Hinvs, rb, bb = K.fov_case(257, 2)
    H = Hinvs[0]
    local = pts.dot(H[:3, :3].T) + H[:3, 3]
    want = (np.linalg.norm(local, axis=1) < rb[0]) & (abs(np.arctan2(local[:, 1], local[:, 0])) < bb[0])
    got = store.fov3_numpy(pts, H, rb[0], bb[0])
    assert got.dtype == bool and np.array_equal(got, want) and 0 < got.sum() < len(pts)
    # the bearing is the horizontal one: z changes the range only
    up = pts.copy()
    up[:, 2] += 1.0
    assert np.array_equal(store.fov3_numpy(up, R.EYE, np.inf, 1.0), store.fov3_numpy(pts, R.EYE, np.inf, 1.0))


def test_symbols_signatures_and_header_agree():
    hdr = open(os.path.join(ROOT, "include", "sonarfe.h")).read()
    lib = L.load_library()
    for name in NEW:
        assert name in L.SIGNATURES and hasattr(lib, name) and "int " + name + "(" in hdr, name
        proto = hdr[hdr.index("int " + name + "("):]
        proto = proto[:proto.index(";")]
        assert proto.count(",") + 1 == len(L.SIGNATURES[name][1]), name
    assert "Not provided in 3-D: keyed clouds" not in hdr


def test_null_context_is_an_error_before_any_device_call():
    lib = L.load_library()
    h = ctypes.c_int32(7)
    n = ctypes.c_int(7)
    assert lib.sfe_cloud_store3_put_keys(None, None, 0, None, None, 0, ctypes.byref(h)) < 0 and h.value == 7
    assert lib.sfe_cloud_store3_keyed(None, 0) < 0
    assert lib.sfe_cloud_store3_get_points_keys(None, None, None, None, None, None, 0, 0.5, None, None) < 0
    assert lib.sfe_cloud_store3_read_keys(None, None, 0, None, 0, ctypes.byref(n)) < 0 and n.value == 7
    assert lib.sfe_cloud_store3_fov_select(None, None, None, 0, None, None, None, None, 0, None, None, None) < 0
    assert lib.sfe_cloud_store3_set_selection(None, None, 0, None, 0) < 0
    assert lib.sfe_cloud_store3_compact_selected(None, None, None, 0, None, None) < 0
    assert lib.sfe_cloud_store3_match_keys(None, None, None, None, 0, 1.0, 0, None, None) < 0


def _build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + extra +
                   [os.path.join(ROOT, "tests", "host", "store3_keys_check.cpp"), "-o", exe], check=True, timeout=180)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, universal_newlines=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("store3_keys_check: ok"), r.stdout[-2000:]


def test_keys_check_builds_and_passes(tmp_path):
    _build(tmp_path, "store3_keys_check", [])


def test_keys_check_under_sanitizers(tmp_path):
    """the same program with the address and undefined-behaviour sanitizers, as a stand-alone program"""
    _build(tmp_path, "store3_keys_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
