"""CPU: the 3-D ICP chains (data-point filters, MinDist / MedianDist, Bound on N x 3 clouds) without a device.

- ``parse_icp_chain(text, dims=3)`` takes ``dim: 2`` and z bounds and returns a ``dims = 3`` chain; with the default it
  refuses them as before.  ``dims`` round-trips through ``as_dict`` / ``from_dict``; a 2-D chain's dictionary is unchanged.
- The refusals: a ``dims = 2`` chain with filters or modules on N x 3 clouds (today's words), a ``dims = 3`` chain on N x 2
  clouds; neither reaches a library call.
- tests/host/icp3_chain_check.cpp evaluates sfe_icp3_chain.h (stage predicates, keep test, Bound test, validation) on
  boundary inputs, plain and under the address / undefined-behaviour sanitizers; its output equals ``dpf3_ref`` /
  ``icp3_chain_ref`` bit for bit.
- On the reference alone: z = 0 clouds with planar guesses give ``icp_chain_ref.icp``'s status and iterations; every
  constructed case moves the result of the shipped chain; for every boundary case the named wrong variant differs.
"""
import os
import subprocess

import numpy as np
import pytest

from sonar_slam_amd import _lib as L
from sonar_slam_amd import icp_config, pcl, store

import dpf3_ref as D
import icp3_cases as C3
import icp3_chain_cases as C
import icp3_chain_ref as R
import icp3_ref
import icp_chain_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

YAML3 = """
readingDataPointsFilters:
  - MaxDistDataPointsFilter:
      dim: 2
      maxDist: 1.5
  - MinDistDataPointsFilter:
      dim: -1
      minDist: 0.25
referenceDataPointsFilters:
  - BoundingBoxDataPointsFilter:
      xMin: -3
      xMax: 3
      yMin: -4
      yMax: 4
      zMin: -0.5
      zMax: 2.5
      removeInside: 0
  - OctreeGridDataPointsFilter:
      maxSizeByNode: 0.2
      samplingMethod: 3
matcher:
  KDTreeMatcher:
    knn: 1
    maxDist: 10
outlierFilters:
  - MedianDistOutlierFilter:
      factor: 3
  - MinDistOutlierFilter:
      minDist: 0.01
errorMinimizer:
  PointToPointErrorMinimizer
transformationCheckers:
  - CounterTransformationChecker:
      maxIterationCount: 30
  - BoundTransformationChecker:
      maxRotationNorm: 0.8
      maxTranslationNorm: 4
inspector:
  NullInspector
logger:
  NullLogger
"""


def test_parse_takes_the_z_axis_only_for_a_3d_chain():
    ch = icp_config.parse_icp_chain(YAML3, dims=3)
    assert ch.dims == 3 and ch.reading[0].dim == 2 and ch.reading[0].kind == L.DPF_MAX_DIST
    assert list(ch.reference[0].f) == [-3.0, 3.0, -4.0, 4.0, -0.5, 2.5] and ch.reference[0].remove_inside == 0
    assert ch.outliers.use_median and ch.outliers.use_min_dist and ch.outliers.use_bound and ch.outliers.bound_order == 1
    with pytest.raises(icp_config.IcpConfigError, match="3-D"):
        icp_config.parse_icp_chain(YAML3)
    with pytest.raises(icp_config.IcpConfigError, match="3-D"):
        icp_config.parse_icp_chain(YAML3, dims=2)
    for bad in ("dim: 3", "dim: -2"):
        with pytest.raises(icp_config.IcpConfigError, match="not -1, 0, 1 or 2"):
            icp_config.parse_icp_chain(YAML3.replace("dim: 2", bad), dims=3)
    with pytest.raises(icp_config.IcpConfigError, match="dims"):
        icp_config.parse_icp_chain(YAML3, dims=4)
    # a chain without a z axis parses either way and differs in dims alone
    flat = YAML3.replace("dim: 2", "dim: 1")
    a, b = icp_config.parse_icp_chain(flat), icp_config.parse_icp_chain(flat, dims=3)
    assert a.dims == 2 and b.dims == 3 and a != b
    b.dims = 2
    assert a == b


def test_dims_round_trips_and_a_2d_dictionary_is_unchanged():
    ch3 = icp_config.parse_icp_chain(YAML3, dims=3)
    d = ch3.as_dict()
    assert d["dims"] == 3
    back = icp_config.IcpChain.from_dict(d)
    assert back == ch3 and back.dims == 3 and "dims=3" in repr(ch3).replace("'dims': 3", "dims=3")
    ch2 = icp_config.IcpChain(icp_config.shipped_params(), reading=[D.max_dist(20.0)])
    assert ch2.dims == 2 and sorted(ch2.as_dict()) == ["outliers", "params", "reading", "reference"]
    assert icp_config.IcpChain.from_dict(ch2.as_dict()) == ch2
    assert icp_config.IcpChain(icp_config.shipped_params(), dims=3) != icp_config.IcpChain(icp_config.shipped_params())
    with pytest.raises(icp_config.IcpConfigError):
        icp_config.IcpChain(icp_config.shipped_params(), dims=1)


class _NoDevice(object):
    """a context that fails the test if a refused call reaches the library"""
    def __getattr__(self, name):
        raise AssertionError("the call reached the device context (%s)" % name)


def test_refusals_by_dimension_reach_no_library_call():
    icp = pcl.ICP(_NoDevice())
    s3, t3, g4 = np.zeros((5, 3), f32), np.ones((6, 3), f32), np.eye(4, dtype=f32)
    s2, t2, g3 = np.zeros((5, 2), f32), np.ones((6, 2), f32), np.eye(3, dtype=f32)
    p = icp_config.shipped_params()
    # a dims = 2 chain on N x 3 clouds: today's words
    for chain, what in ((icp_config.IcpChain(p, reading=[D.max_dist(20.0)]), "data-point filters"),
                        (icp_config.IcpChain(p, outliers=L.IcpOutliers(use_median=1, median_factor=3.0)), "MedianDist")):
        icp.setChain(chain)
        for call in (lambda: icp.compute(s3, t3, g4), lambda: icp.compute_batch(s3, t3, [g4, g4]),
                     lambda: icp.compute_pairs([s3], [t3], [g4]),
                     lambda: icp.compute_jobs(s3, t3, [[0, 5, 0, 6]], g4.reshape(1, 16))):
            with pytest.raises(NotImplementedError, match=what):
                call()
    # a dims = 3 chain on N x 2 clouds, with or without modules
    for chain in (C.chain3(p), C.chain3(p, reading=[D.max_dist(1.0, 2)]), C.chain3(p, use_median=1, median_factor=3.0)):
        icp.setChain(chain)
        for call in (lambda: icp.compute(s2, t2, g3), lambda: icp.compute_batch(s2, t2, [g3]),
                     lambda: icp.compute_pairs([s2], [t2], [g3]),
                     lambda: icp.compute_jobs(s2, t2, [[0, 5, 0, 6]], g3.reshape(1, 9))):
            with pytest.raises(NotImplementedError, match="dims = 3"):
                call()
    # a stage on the z axis in a chain that claims to be 2-D
    icp.setChain(icp_config.IcpChain(p, reading=[D.max_dist(1.0, 2)]))
    with pytest.raises(NotImplementedError, match="dim: 2"):
        icp.compute(s2, t2, g3)
    # the store route repeats the 2-D chain's refusal and takes the 3-D chain's arguments from the same place
    st = store.CloudStore3.__new__(store.CloudStore3)
    st.ctx, st.handle = _NoDevice(), None
    with pytest.raises(NotImplementedError, match="data-point filters"):
        st.icp(np.array([[0, 1]], np.int32), g4[None], icp_config.IcpChain(p, reference=[D.octree(0.5)]))


def test_a_3d_chain_without_modules_takes_the_plain_entry_point():
    icp = pcl.ICP(_NoDevice())
    icp.setChain(C.chain3(icp_config.shipped_params(minimizer=2)))
    assert icp._chain3("x").minimizer == 2 and icp._ext3() is None
    icp.setChain(C.chain3(icp_config.shipped_params(), reference=[D.octree(0.5)], use_bound=1, max_rotation_norm=1.0,
                          max_translation_norm=1.0))
    ext = icp._ext3()
    assert ext is not None and len(ext) == 5 and ext[1:3] == (None, 0) and ext[4] == 1
    for name in ("sfe_icp3_filter_clouds_dev", "sfe_icp3_compute_jobs_chain_ext", "sfe_icp3_store_compute_chain_ext"):
        assert name in L.SIGNATURES and hasattr(L.load_library(), name)
        assert name + "(" in open(os.path.join(ROOT, "include", "sonarfe.h")).read()
    assert len(L.SIGNATURES["sfe_icp3_compute_jobs_chain_ext"][1]) == 17
    assert len(L.SIGNATURES["sfe_icp3_store_compute_chain_ext"][1]) == 14
    lib = L.load_library()
    assert lib.sfe_icp3_filter_clouds_dev(None, None, 0, None, None, 0, None, None) < 0
    assert lib.sfe_icp3_compute_jobs_chain_ext(None, None, None, None, 0, None, 0, None, 0, None, 0, None, None, 0, None, None,
                                               None) < 0
    assert lib.sfe_icp3_store_compute_chain_ext(None, None, None, None, 0, None, 0, None, None, None, 0, None, None, None) < 0


# ---- the host program against the numpy restatement ---------------------------------------------------------------------
def _hex(v):
    v = float(f32(v))
    return "nan" if np.isnan(v) else ("inf" if v > 0 else "-inf") if np.isinf(v) else v.hex()


def _around(v):
    v = f32(v)
    return [np.nextafter(v, f32(-np.inf)), v, np.nextafter(v, f32(np.inf))]


def _boundary_inputs():
    """-> (lines for the program, expected output lines)"""
    lines, want = [], []

    def pred(st, pt):
        lines.append("P %d %d %d %s %s" % (st.kind, st.dim, st.remove_inside, " ".join(_hex(v) for v in st.f),
                                          " ".join(_hex(v) for v in pt)))
        want.append("P %d" % int(D.keep_mask(np.asarray([pt], f32), st)[0]))

    special = [f32(np.nan), f32(np.inf), f32(-np.inf), f32(0.0), f32(-0.0)]
    thr = f32(1.7)
    for dim in (0, 1, 2):                          # a coordinate on the threshold and one ulp either side, both signs
        for v in _around(thr) + _around(-thr) + special:
            pt = [f32(0.3), f32(-0.2), f32(0.1)]
            pt[dim] = v
            for st in (D.max_dist(thr, dim), D.min_dist(thr, dim), D.max_dist(-thr, dim), D.min_dist(-thr, dim)):
                pred(st, pt)
    # the norm on the threshold and one ulp either side: (1.5, 2, 0) has norm 2.5 exactly, so has (0, 1.5, 2)
    for pt in ([1.5, 2.0, 0.0], [0.0, 1.5, 2.0], [2.0, 0.0, -1.5], [0.7, -1.1, 2.3], [np.nan, 0, 0], [0, np.inf, 0],
               [0, 0, -np.inf], [3e19, 3e19, 3e19], [1e-30, 1e-30, 1e-30]):
        pt = [f32(v) for v in pt]
        n = D.norm(*pt)
        lines.append("N " + " ".join(_hex(v) for v in pt))
        want.append("N %08x" % int(np.asarray(n, f32).view(np.uint32)))
        for t in (_around(n) if np.isfinite(n) else [f32(1.0), f32(np.inf)]):
            for st in (D.max_dist(t), D.min_dist(t), D.max_dist(-t), D.min_dist(-t)):
                pred(st, pt)
    # a box bound on each of the six faces, one ulp either side, inside kept and inside removed
    lo, hi = (f32(-1.25), f32(-2.5), f32(0.5)), (f32(3.0), f32(-0.75), f32(4.5))
    mid = [f32(0.5), f32(-1.5), f32(2.0)]
    for a in range(3):
        for face in (lo[a], hi[a]):
            for v in _around(face) + special[:3]:
                pt = list(mid)
                pt[a] = v
                for ri in (0, 1):
                    pred(D.box(lo, hi, ri), pt)
    # the keep test of the outlier filters on the threshold and one ulp either side
    for d in _around(C.T2) + [f32(np.inf), f32(0.0)]:
        for use_min, use_med in ((1, 0), (0, 1), (1, 1), (0, 0)):
            ox = L.IcpOutliers(use_min_dist=use_min, min_dist=1.5, use_median=use_med, median_factor=2.25)
            lim = f32(f32(2.25) * f32(1.0))
            lines.append("O %d %s %d %s %s %s" % (use_min, _hex(1.5), use_med, _hex(2.25), _hex(1.0), _hex(d)))
            want.append("O %d %08x %08x" % (int(R.ox_keep(ox, np.asarray([d], f32), lim)[0]),
                                           int(np.asarray(f32(1.5) * f32(1.5), f32).view(np.uint32)),
                                           int(np.asarray(lim, f32).view(np.uint32))))
    for n in (1, 2, 3, 80, 81, 124, 16777217, 33554435):
        lines.append("M %d" % n)
        want.append("M %d" % R.median_rank(n))
    # Bound: a rotation angle and a translation norm at the bound and just beside it
    T = np.asarray(C3.rigid((0.3, -0.5, 0.8), 0.4, (0.3, -1.2, 0.4)), f32)
    rot, tr = R.bound_rot(T), R.bound_trans(T)
    cases = [(T, r_, t_) for r_ in _around(rot) + [f32(10.0)] for t_ in _around(tr) + [f32(10.0)]]
    half = np.asarray(C3.rigid((0, 1, 0), np.pi, (0, 0, 0)), f32)          # trace < 0: the other quaternion branch
    nan_t = T.copy()
    nan_t[0, 3] = np.nan
    nan_r = T.copy()
    nan_r[1, 1] = np.nan
    cases += [(np.eye(4, dtype=f32), f32(1e-3), f32(1e-3)), (half, f32(3.0), f32(1.0)), (half, f32(3.2), f32(1.0)),
              (nan_t, f32(10.0), f32(1e-3)), (nan_r, f32(1e-3), f32(10.0))]
    for M, r_, t_ in cases:
        ox = L.IcpOutliers(use_bound=1, max_rotation_norm=r_, max_translation_norm=t_)
        lines.append("B %s %s %s" % (_hex(r_), _hex(t_), " ".join(_hex(v) for v in M.reshape(-1))))
        want.append("B %d %s %s" % (int(R.bound_out(ox, M)), R.bound_rot(M), R.bound_trans(M)))
    # the validation of a stage list
    ok = (L.DPF_MAX_DIST, 2, 1.0)
    for stages, code, bad in (([ok, (L.DPF_MIN_DIST, -1, 1.0), (L.DPF_BOUNDING_BOX, 7, 0.0), (L.DPF_OCTREE_GRID, -1, 0.5)], 0, 4),
                              ([ok, (L.DPF_MAX_DIST, 3, 1.0)], 2, 1), ([(L.DPF_MIN_DIST, -2, 1.0)], 2, 0),
                              ([ok, ok, (L.DPF_OCTREE_GRID, -1, 0.0)], 3, 2), ([(L.DPF_OCTREE_GRID, -1, -1.0)], 3, 0),
                              ([(L.DPF_OCTREE_GRID, -1, np.nan)], 3, 0), ([(L.DPF_OCTREE_GRID, -1, np.inf)], 3, 0),
                              ([(9, 0, 1.0)], 4, 0), ([ok] * L.DPF_MAX_STAGES, 0, L.DPF_MAX_STAGES),
                              ([ok] * (L.DPF_MAX_STAGES + 1), 1, L.DPF_MAX_STAGES + 1), ([], 0, 0)):
        lines.append("V %d %s" % (len(stages), " ".join("%d %d %s" % (k, d, _hex(v)) for k, d, v in stages)))
        want.append("V %d %d" % (code, bad))
    return lines, want


def _run_check(tmp_path, name, extra):
    exe, inp = str(tmp_path / name), str(tmp_path / (name + ".in"))
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + extra +
                   [os.path.join(ROOT, "tests", "host", "icp3_chain_check.cpp"), "-o", exe], check=True, timeout=180)
    lines, want = _boundary_inputs()
    with open(inp, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, inp], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, universal_newlines=True)
    got = r.stdout.strip().split("\n")
    assert r.returncode == 0 and got[-1] == "icp3_chain_check: ok (%d lines)" % len(lines), r.stdout[-2000:]
    assert len(got) - 1 == len(want) > 300
    for i, (g, w) in enumerate(zip(got, want)):
        if w[0] == "B":                            # the doubles by value: "%a" and repr spell them differently
            gt, wt = g.split(), w.split()
            same = gt[:2] == wt[:2] and all(
                (np.isnan(float.fromhex(a)) and np.isnan(float(b))) or float.fromhex(a) == float(b)
                for a, b in zip(gt[2:], wt[2:]))
        else:
            same = g == w
        assert same, (i, lines[i], g, w)
    kinds = set(w.split()[0] + w.split()[1] for w in want if w[0] in "PO")
    assert kinds == {"P0", "P1", "O0", "O1"}


def test_chain_check_builds_and_matches_the_restatement(tmp_path):
    _run_check(tmp_path, "icp3_chain_check", [])


def test_chain_check_under_sanitizers(tmp_path):
    """the same program with the address and undefined-behaviour sanitizers, as a stand-alone program"""
    _run_check(tmp_path, "icp3_chain_check_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


# ---- on the reference alone -----------------------------------------------------------------------------------------------
def test_planar_clouds_reproduce_the_2d_chain_reference():
    ox = L.IcpOutliers(use_min_dist=1, min_dist=0.004, use_median=1, median_factor=2.0, use_bound=1, max_rotation_norm=1.0,
                       max_translation_norm=5.0, bound_order=3)
    for seed, over in ((11, {}), (12, dict(use_trimmed_filter=0)), (13, dict(max_iter=3))):
        src, tgt, g4 = C3.planar_pair(seed, 300, 350)
        p = icp_config.shipped_params(**over)
        s3, T3, i3 = R.icp(src, tgt, g4, p, ox)
        s2, T2, i2 = icp_chain_ref.icp(src[:, :2], tgt[:, :2], C3.guess3(g4), p, ox)
        assert (s3, i3) == (s2, i2) and s3 == 0 and i3 >= 3
        assert np.abs(C3.guess3(T3) - T2).max() < 1e-5
    # ... and a Bound that stops both, by rotation and by translation
    src, tgt, g4 = C3.planar_pair(11, 300, 350)
    for lim in (dict(max_rotation_norm=0.005, max_translation_norm=5.0), dict(max_rotation_norm=1.0, max_translation_norm=0.01)):
        ob = L.IcpOutliers(use_bound=1, bound_order=0, **lim)
        s3, T3, i3 = R.icp(src, tgt, g4, icp_config.shipped_params(), ob)
        s2, _, i2 = icp_chain_ref.icp(src[:, :2], tgt[:, :2], C3.guess3(g4), icp_config.shipped_params(), ob)
        assert (s3, i3) == (s2, i2) and s3 == 9 and np.array_equal(T3, g4)


def test_without_modules_the_chain_reference_is_the_shipped_one():
    src, tgt, g = C.pair(21, 260, 300)
    for m, ref in ((0, icp3_ref.icp), (2, None)):
        p = icp_config.shipped_params(minimizer=m)
        got = R.icp(src, tgt, g, p)
        if ref is None:
            import icp3_plane_ref
            ref = icp3_plane_ref.icp
        want = ref(src, tgt, g, p)
        assert got[0] == want[0] == 0 and got[2] == want[2] and np.array_equal(got[1], want[1])
        same = R.icp(src, tgt, g, p, L.IcpOutliers(use_min_dist=1, min_dist=0.0))
        assert same[0] == 0 and same[2] == want[2] and np.array_equal(same[1], want[1])


def test_every_constructed_case_moves_the_shipped_result():
    """a module dropped silently cannot pass: each case's result differs from the same job without the module"""
    tgt, (src, grp) = C.lattice_target(), C.lattice_source()
    p, I = C.lattice_params(), np.eye(4, dtype=f32)
    plain = R.icp(src, tgt, I, p)
    assert plain[0] == 0 and plain[2] == 1
    for ox in (C.MIN_DIST_ON, C.MEDIAN_ON):
        got = R.icp(src, tgt, I, p, L.IcpOutliers(**ox))
        assert got[0] == 0 and got[2] == 1 and np.abs(got[1] - plain[1]).max() > 1e-3
    src, tgt, g = C.pair(22, 300, 320, n_out=30)
    p = icp_config.shipped_params()
    plain = R.icp(src, tgt, g, p)
    for ox in (dict(use_min_dist=1, min_dist=0.01), dict(use_median=1, median_factor=1.0)):
        got = R.icp(src, tgt, g, p, L.IcpOutliers(**ox))
        assert got[0] == plain[0] == 0 and np.abs(got[1] - plain[1]).max() > 1e-5, ox
    for lim in (dict(max_rotation_norm=0.01, max_translation_norm=5.0), dict(max_rotation_norm=1.0, max_translation_norm=0.02)):
        got = R.icp(src, tgt, g, p, L.IcpOutliers(use_bound=1, **lim))
        assert got[0] == 9 and np.array_equal(got[1], g) and 1 <= got[2] <= plain[2]
    far = R.icp(C.far_source(50), tgt, g, icp_config.shipped_params(use_trimmed_filter=0),
                L.IcpOutliers(use_median=1, median_factor=3.0))
    none = R.icp(C.far_source(50), tgt, g, icp_config.shipped_params(use_trimmed_filter=0))
    assert far[0] == 1 and none[0] == 2 and far[2] == none[2] == 0


def test_the_lattice_distances_are_exact_and_sit_on_the_thresholds():
    tgt, (src, grp) = C.lattice_target(), C.lattice_source()
    tr = []
    R.icp(src, tgt, np.eye(4, dtype=f32), C.lattice_params(), trace=tr)
    ids, d2, _ = tr[0]
    for g, want in ((0, C.T2), (1, C.T2 + C.ULP), (2, C.T2 - C.ULP), (3, 0.25), (4, 1.0), (5, 4.0), (6, np.inf)):
        assert (d2[grp == g] == f32(want)).all(), g
    assert np.nextafter(C.T2, f32(4)) == C.T2 + C.ULP and np.nextafter(C.T2, f32(0)) == C.T2 - C.ULP
    fin = np.sort(d2[ids >= 0])
    assert len(fin) == 80 and fin[R.median_rank(80)] == 1.0 and np.sort(d2)[R.median_rank(len(d2))] == C.T2 - C.ULP


def test_each_wrong_variant_differs_on_its_boundary_case():
    tgt, (src, grp) = C.lattice_target(), C.lattice_source()
    p, I = C.lattice_params(), np.eye(4, dtype=f32)

    def kept(ox, wrong=None):
        tr = []
        out = R.icp(src, tgt, I, p, L.IcpOutliers(**ox), wrong=wrong, trace=tr)
        return out, [int(tr[0][2][grp == g].sum()) for g in range(7)]

    right, k = kept(C.MIN_DIST_ON)
    assert k == [3, 3, 0, 0, 0, 10, 0]
    wrong, kw = kept(C.MIN_DIST_ON, "min_strict")
    assert kw == [0, 3, 0, 0, 0, 10, 0] and np.abs(wrong[1] - right[1]).max() > 1e-3
    right, k = kept(C.MEDIAN_ON)
    assert k == [3, 0, 3, 40, 21, 0, 0]
    wrong, kw = kept(C.MEDIAN_ON, "median_all")
    assert kw == [3, 3, 3, 40, 21, 10, 0] and np.abs(wrong[1] - right[1]).max() > 1e-3
    # Bound listed behind a Counter that ends the job at its first iteration: the job succeeds; checked first, it stops it
    ob = dict(use_bound=1, max_rotation_norm=1e-4, max_translation_norm=1e-4, bound_order=1)
    assert kept(ob)[0][0] == 0 and kept(ob, "bound_first")[0][0] == 9
    assert kept(dict(ob, bound_order=0))[0][0] == 9 and kept(dict(ob, bound_order=2))[0][0] == 9
