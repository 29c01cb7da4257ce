"""CPU: the 3-D ICP's numpy restatement (tests/icp3_ref.py), the one-lane solve of the kernel (sfe_icp3_solve.h, through
tests/host/icp3_solve_check.cpp), the inputs of the GPU tests (tests/icp3_cases.py) and the refusals of ``pcl.ICP``.

- z = 0 clouds with embedded guesses: icp3_ref reports icp_chain_ref's status and iterations and its pose, embedded, within
  1e-6 (shipped parameters, trimmed ratio 0.5, max_iter reached).
- Reflection fix.  On exactly planar input H is block diagonal and U V^T of ``np.linalg.svd`` comes back proper (the null
  vectors of U and V agree), so removing the fix changes nothing there: measured, 0 reflections in every step of the z = 0
  cases.  The inputs that need it are the nearly planar ones (``icp3_cases.thin_jobs``): there the fix fires and the
  reference without it misses the bar.  Both facts are asserted; the GPU tests run the thin jobs too.
- A random cloud moved by a known rigid motion about a skew axis, noise-free, is recovered within 1e-4.
- Every input of the GPU tests: the reference with its fp64 sums in reversed point order lands within 1e-7 of itself with
  equal status and iterations; coordinates within +-4 m; the cases built for a tie, a run of equal distances, a status or a
  stop have them.
- icp3_solve_check against numpy: R within 1e-12 per entry over random H, planar H and H that need the reflection fix, all
  with a conditioning of at least 1e-3 ((s2 + s3) / s1, s3 counted negative where det H < 0: that is what the polar
  rotation's error grows with); quaternion distances for all four branches of Eigen's rule.
- Refusals of pcl.ICP on 3-D input, and the 2-D entry points still refuse what they refused.
"""
import os
import subprocess

import numpy as np
import pytest

from sonar_slam_amd import _lib as L
from sonar_slam_amd import icp_config, pcl

import icp3_cases as C
import icp3_ref
import icp_chain_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_TIGHT = 1e-6          # the bar of tests/test_gpu_icp_outliers.py
f32 = np.float32


def _diff(Ta, Tb):
    return float(np.abs(np.asarray(Ta, np.float64) - np.asarray(Tb, np.float64)).max())


# ---- z = 0 against the 2-D reference ----
@pytest.mark.parametrize("k", range(3))
def test_planar_input_gives_the_2d_reference(k):
    s, t, g, p = C.planar_jobs()[k]
    st2, T2, it2 = icp_chain_ref.icp(s[:, :2], t[:, :2], C.guess3(g), p)
    stats = {}
    st3, T3, it3 = icp3_ref.icp(s, t, g, p, stats=stats)
    assert (st3, it3) == (st2, it2) and st2 == 0
    if k == 2:
        assert it3 == p.max_iter                      # the Counter checker stopped it
    assert _diff(T3, icp3_ref.embed(T2)) < TOL_TIGHT
    # exactly planar input never needs the reflection fix (see the module docstring) ...
    assert stats.get("reflections", 0) == 0
    assert _diff(icp3_ref.icp(s, t, g, p, reflection_fix=False)[1], T3) == 0.0


def test_nearly_planar_input_needs_the_reflection_fix():
    # ... nearly planar input does: without the fix the reference misses the bar
    fired, missed = 0, 0
    for s, t, g, p in C.thin_jobs():
        stats = {}
        st, T, it = icp3_ref.icp(s, t, g, p, stats=stats)
        assert st == 0 and _diff(T, C.TRUTH) < 5e-3   # (5 mm of noise on 400 points)
        assert abs(np.linalg.det(T[:3, :3].astype(np.float64)) - 1.0) < 1e-5
        fired += stats.get("reflections", 0) > 0
        bad = icp3_ref.icp(s, t, g, p, reflection_fix=False)
        if _diff(bad[1], T) > TOL_TIGHT:
            assert stats.get("reflections", 0) > 0
            missed += 1
    assert fired >= 2 and missed >= 2, (fired, missed)


def test_known_rigid_motion_about_a_skew_axis_is_recovered():
    rng = np.random.default_rng(5)
    tgt = (rng.uniform(-1, 1, (600, 3)) * np.array([3.0, 3.0, 2.0])).astype(f32)
    truth = C.rigid(C.SKEW, 0.2, (0.25, -0.2, 0.15))
    src = C.apply(np.linalg.inv(truth), tgt.astype(np.float64)).astype(f32)
    guess = np.asarray(C.rigid((0.1, 0.9, 0.2), 0.04, (0.05, -0.04, 0.06)) @ truth, f32)
    st, T, it = icp3_ref.icp(src, tgt, guess, C.params())
    assert st == 0 and _diff(T, truth) < 1e-4, (st, it, _diff(T, truth))


# ---- the inputs of the GPU tests ----
@pytest.mark.parametrize("name", sorted(C.all_jobs()))
def test_gpu_input_is_stable_under_the_order_of_the_sums(name):
    s, t, g, p = C.job(name)
    fin = np.isfinite(s)
    assert np.abs(s[fin]).max(initial=0.0) <= 4.0 and np.abs(t).max() <= 4.0
    a = C.ref(name)
    b = icp3_ref.icp(s, t, g, p, reverse_sums=True)
    assert (a[0], a[2]) == (b[0], b[2])
    if a[0] == 0:
        assert _diff(a[1], b[1]) < 1e-7
    else:
        assert np.array_equal(a[1], g, equal_nan=True)


def test_tie_case_depends_on_the_lowest_index():
    (s, t, g, p), ties = C.tie_case()
    assert float(np.cumsum(t.astype(np.float64), axis=0)[-1].max()) == 0.0          # the mean is exactly zero
    lo_tr, hi_tr = [], []
    a = icp3_ref.icp(s, t, g, p, trace=lo_tr)
    b = icp3_ref.icp(s, t, g, p, tie_high=True, trace=hi_tr)
    for q, lo, hi in ties:
        assert lo_tr[0][0][q] == lo and hi_tr[0][0][q] == hi and lo_tr[0][1][q] == hi_tr[0][1][q]
        assert lo_tr[0][2][q]                                                       # kept by the filters
        assert lo // C.TILE != hi // C.TILE or q == 1
    assert a[0] == 0 and b[0] == 0 and _diff(a[1], b[1]) > 100 * TOL_TIGHT
    # each tie alone moves the pose beyond the bar: the other choice for one query, the right one for the rest
    for q, lo, hi in ties:
        t2 = t.copy()
        t2[[lo, hi]] = t[[hi, lo]]
        assert _diff(icp3_ref.icp(s, t2, g, p)[1], a[1]) > 100 * TOL_TIGHT


def test_quantile_cases_land_on_a_run_of_equal_distances():
    for s, t, g, p in C.quantile_run_jobs():
        tr = []
        icp3_ref.icp(s, t, g, p, trace=tr)
        ids, d2, keep = tr[0]
        vals, counts = np.unique(d2, return_counts=True)
        assert list(counts) == [20, 100, 20]
        n = len(d2)
        k = n - 1 if p.trim_ratio >= 1.0 else int(f32(n) * f32(p.trim_ratio))
        assert np.sort(d2)[k] == (vals[2] if p.trim_ratio >= 1.0 else vals[1])
        assert keep.sum() == (140 if p.trim_ratio >= 1.0 else 120)


def test_status_cases_report_what_they_are_built_for():
    want = {"no_finite_distance": 1, "all_sources_nan": 1, "max_dist_drops_all": 2}
    for name, st in want.items():
        assert C.ref(name)[0] == st and C.ref(name)[2] == 0, name
    # A NaN in the guess reaches every moved source point through T0 (a product with NaN is NaN, also with a zero of
    # translate(-mean)): no distance is finite and the trimmed filter reports status 1 before a transform is checked
    assert C.ref("nan_in_guess")[0] == 1
    smooth = C.params().smooth_len
    assert C.ref("counter_below_smooth")[2] == 2 < smooth
    assert C.ref("counter_above_smooth")[2] == 6 > smooth
    assert C.ref("diff_at_smooth")[2] == smooth          # the first step at which the checker has smoothLength differences
    assert C.ref("diff_above_smooth")[2] > smooth + 1 and C.ref("diff_above_smooth")[2] < C.params().max_iter
    assert C.ref("longer_than_history")[2] == C.MAX_HIST + 16
    tr = []
    s, t, g, p = C.nonfinite_job()
    icp3_ref.icp(s, t, g, p, trace=tr)
    assert 0 < (tr[0][0] >= 0).sum() <= len(s) - 25       # NaN, infinite and far sources have no match
    srcs, tgts, jobs, p = C.mixed_launch()
    assert [C.ref("mixed%d" % k)[0] for k in range(len(jobs))] == [0, 0, 2, 0, 0, 0, 0, 0]


# ---- the kernel's one-lane arithmetic against numpy ----
@pytest.fixture(scope="module")
def solve_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("icp3") / "icp3_solve_check")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                    os.path.join(ROOT, "tests", "host", "icp3_solve_check.cpp"), "-o", exe], check=True, timeout=120)

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120,
                           universal_newlines=True)
        out = r.stdout.strip().split("\n")
        assert r.returncode == 0 and out[-1] == "icp3_solve_check: ok", r.stdout[-2000:]
        assert len(out) == len(lines) + 1
        return [np.array([float(v) for v in ln.split()]) for ln in out[:-1]]
    return run


def _fmt(kind, v):
    return kind + " " + " ".join("%.17g" % x for x in np.ravel(v))


def _rot(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def _some_H(rng, kind):
    """H = U diag(s) V^T with proper U, V; 'reflect': det H < 0.  Conditioning (s2 + s3') / s1 >= 1e-3, s3' the signed s3."""
    s1 = 10.0 ** rng.uniform(-3, 3)
    s2 = s1 * 10.0 ** rng.uniform(-2.5, 0)
    if kind == "planar":
        s3 = 0.0
    elif kind == "reflect":
        s3 = -s2 * rng.uniform(0.0, 0.5)
    else:
        s3 = s2 * rng.uniform(0.0, 1.0)
    assert (s2 + s3) / s1 >= 1e-3
    return _rot(rng) @ np.diag([s1, s2, s3]) @ _rot(rng).T


def test_solve_agrees_with_numpy(solve_check):
    rng = np.random.default_rng(11)
    Hs = [_some_H(rng, kind) for kind in ("random", "planar", "reflect") for _ in range(200)]
    z = np.zeros((3, 3))
    z[:2, :2] = _some_H(rng, "random")[:2, :2]
    Hs.append(z)                                           # exactly block diagonal, as z = 0 clouds give it
    stats = {}
    want = [icp3_ref.rotation(H, stats=stats) for H in Hs]
    assert stats["reflections"] >= 200
    got = solve_check([_fmt("H", H) for H in Hs])
    worst = max(float(np.abs(g.reshape(3, 3) - w).max()) for g, w in zip(got, want))
    assert worst < 1e-12, worst
    # sums -> (R, t)
    accs = []
    for _ in range(50):
        n = int(rng.integers(3, 40))
        P, Q = rng.uniform(-4, 4, (n, 3)), rng.uniform(-4, 4, (n, 3))
        accs.append(np.concatenate([[n], P.sum(0), Q.sum(0), (Q[:, :, None] * P[:, None, :]).sum(0).ravel()]))
    got = solve_check([_fmt("S", a) for a in accs])
    for g, a in zip(got, accs):
        H = a[7:].reshape(3, 3) - np.outer(a[4:7], a[1:4] / a[0])
        s = np.linalg.svd(H, compute_uv=False)
        if (s[1] + np.sign(np.linalg.det(H)) * s[2]) / s[0] < 1e-3:
            continue
        R, t = icp3_ref.solve(a)
        assert np.abs(g[:9].reshape(3, 3) - R).max() < 1e-12 and np.abs(g[9:] - t).max() < 1e-10


def test_quaternion_distance_agrees_with_numpy(solve_check):
    rng = np.random.default_rng(12)
    blocks = {"trace": C.rigid((1, 2, 3), 0.4, (0, 0, 0))[:3, :3]}
    for i, axis in enumerate(((1, 0.05, -0.03), (0.04, 1, 0.02), (-0.05, 0.03, 1))):
        blocks["diag%d" % i] = C.rigid(axis, 3.0, (0, 0, 0))[:3, :3]        # a turn of almost pi about axis i: trace < 0
    for name, m in blocks.items():
        q = icp3_ref.quat(m.astype(f32))
        branch = 0 if np.trace(m) > 0 else 1 + int(np.argmax(np.diag(m)))
        assert (name == "trace") == (branch == 0) and (branch == 0 or name == "diag%d" % (branch - 1))
        assert abs(np.linalg.norm(q) - 1) < 1e-6
    lines, want = [], []
    names = sorted(blocks)
    for a in names:
        for b in names:
            ma = (blocks[a] @ C.rigid(rng.normal(size=3), 0.01, (0, 0, 0))[:3, :3]).astype(f32)
            mb = blocks[b].astype(f32)
            lines.append(_fmt("Q", np.concatenate([ma.ravel(), mb.ravel()])))
            want.append(np.concatenate([[icp3_ref.quat_dist(icp3_ref.quat(ma), icp3_ref.quat(mb))], icp3_ref.quat(ma),
                                        icp3_ref.quat(mb)]))
    got = solve_check(lines)
    for g, w in zip(got, want):
        assert np.abs(g - w).max() < 1e-13, (g, w)
    # ... and it is the angle between the rotations
    ma, mb = blocks["trace"], blocks["trace"] @ C.rigid((0, 1, 0), 0.3, (0, 0, 0))[:3, :3]
    assert abs(icp3_ref.quat_dist(icp3_ref.quat(ma), icp3_ref.quat(mb)) - 0.3) < 1e-12


def test_solve_check_under_sanitizers(tmp_path):
    """the same program with the address and undefined-behaviour sanitizers, as a stand-alone program"""
    exe = str(tmp_path / "icp3_solve_check_san")
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                    "-Wextra", "-Werror", os.path.join(ROOT, "tests", "host", "icp3_solve_check.cpp"), "-o", exe],
                   check=True, timeout=180)
    rng = np.random.default_rng(13)
    lines = [_fmt("H", _some_H(rng, k)) for k in ("random", "planar", "reflect") for _ in range(20)]
    lines += [_fmt("H", np.zeros(9)), _fmt("H", np.full(9, np.nan)), _fmt("H", np.full(9, np.inf))]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120,
                       universal_newlines=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("icp3_solve_check: ok"), r.stdout[-2000:]


# ---- pcl.ICP: what stays refused ----
class _NoDevice(object):
    """a context that fails the test if a refused call reaches the library"""
    def __getattr__(self, name):
        raise AssertionError("the call reached the device context (%s)" % name)


def _icp(chain=None, **kw):
    icp = pcl.ICP(ctx=_NoDevice())
    if chain is not None:
        icp.setChain(chain)
    else:
        icp.setParams(icp_config.shipped_params(**kw))
    return icp


def test_3d_icp_refusals():
    c3 = np.zeros((5, 3), f32)
    c2 = np.zeros((5, 2), f32)
    e3, e4 = np.eye(3, dtype=f32), np.eye(4, dtype=f32)
    j = np.array([[0, 5, 0, 5]], np.int32)
    icp = _icp()
    for call in (lambda: icp.compute(c3, c3, e3), lambda: icp.compute_batch(c3, c3, [e4, e3]),
                 lambda: icp.compute_pairs([c3], [c3], [e3]), lambda: icp.compute_jobs(c3, c3, j, e3.reshape(1, 9))):
        with pytest.raises(NotImplementedError, match="N x 3 clouds"):
            call()
    for call in (lambda: icp.compute(c2, c2, e4), lambda: icp.compute_batch(c2, c2, [e4]),
                 lambda: icp.compute_pairs([c2], [c2], [e4]), lambda: icp.compute_jobs(c2, c2, j, e4.reshape(1, 16))):
        with pytest.raises(NotImplementedError, match="4 x 4 guesses"):
            call()
    for call in (lambda: icp.compute(c3, c2, e4), lambda: icp.compute(c2, c3, e3), lambda: icp.compute_batch(c2, c3, [e4]),
                 lambda: icp.compute_pairs([c3, c3], [c3, c2], [e4, e4]), lambda: icp.compute_jobs(c3, c2, j, e4.reshape(1, 16))):
        with pytest.raises(NotImplementedError, match="different widths"):
            call()
    calls = (lambda i: i.compute(c3, c3, e4), lambda i: i.compute_batch(c3, c3, [e4]),
             lambda i: i.compute_pairs([c3], [c3], [e4]), lambda i: i.compute_jobs(c3, c3, j, e4.reshape(1, 16)))
    stage = L.IcpDpf(kind=L.DPF_MAX_DIST, dim=-1, remove_inside=0)
    stage.f[0] = 20.0
    chains = [(icp_config.IcpChain(icp_config.shipped_params(), reading=[stage]), "data-point filters"),
              (icp_config.IcpChain(icp_config.shipped_params(), reference=[stage]), "data-point filters"),
              (icp_config.IcpChain(icp_config.shipped_params(), outliers=L.IcpOutliers(use_median=1, median_factor=3.0)),
               "MedianDist"),
              (icp_config.IcpChain(icp_config.shipped_params(minimizer=1)), "PointToPlane")]
    for chain, what in chains:
        for call in calls:
            with pytest.raises(NotImplementedError, match=what):
                call(_icp(chain))
    with pytest.raises(TypeError):
        icp.compute(c3, c3, np.eye(5, dtype=f32))
    # empty clouds raise RuntimeError as in 2-D
    for call in (lambda: icp.compute(np.zeros((0, 3), f32), c3, e4), lambda: icp.compute(c3, np.zeros((0, 3), f32), e4),
                 lambda: icp.compute_pairs([c3, np.zeros((0, 3), f32)], [c3, c3], [e4, e4]),
                 lambda: icp.compute_jobs(c3, c3, np.array([[0, 0, 0, 5]], np.int32), e4.reshape(1, 16))):
        with pytest.raises(RuntimeError, match="empty point cloud"):
            call()
    # result arrays of the 2-D shape never reach the library (it writes 16 floats per job)
    with pytest.raises(TypeError, match="out="):
        icp.compute_jobs(c3, c3, j, e4.reshape(1, 16), out=(np.zeros(1, np.int32), np.zeros((1, 3, 3), f32), np.zeros(1, np.int32)))
    # before a chain is installed: as in 2-D
    with pytest.raises(RuntimeError, match="before loadFromYaml"):
        pcl.ICP(ctx=_NoDevice()).compute(c3, c3, e4)


def test_2d_entry_points_still_refuse():
    c3 = np.zeros((5, 3), f32)
    with pytest.raises(NotImplementedError, match="N x 3 clouds"):
        pcl._cloud(c3, "x")
    with pytest.raises(NotImplementedError, match="4 x 4 guesses"):
        pcl.ICP._guess(np.eye(4, dtype=f32))
    with pytest.raises(TypeError):
        pcl.ICP._guess(np.eye(2, dtype=f32))
    with pytest.raises(TypeError):
        pcl._cloud(np.zeros((5, 4), f32), "x")
    # CloudStore, IcpFarm, FrontEnd and SessionBatch go through these two and stay 2-D
    import inspect

    from sonar_slam_amd import chained, replay
    assert "pcl.ICP._guess" in inspect.getsource(replay) and "pcl.ICP._guess" in inspect.getsource(chained)


def test_header_declares_the_entry_point_and_the_library_exports_it():
    hdr = open(os.path.join(ROOT, "include", "sonarfe.h")).read()
    assert "int sfe_icp3_compute_jobs(sfe_ctx *ctx, const sfe_icp_params *p, const float *src, int n_src_pts" in hdr
    assert "3-D ICP is not provided" not in hdr
    assert "sfe_icp3_compute_jobs" in L.SIGNATURES and hasattr(L.load_library(), "sfe_icp3_compute_jobs")
    # bad arguments come back as SFE_ERR_ARG before anything touches a device
    import ctypes
    lib = L.load_library()
    assert lib.sfe_icp3_compute_jobs(None, None, None, 0, None, 0, None, None, 0, None, None, None) < 0
    assert isinstance(ctypes.sizeof(L.IcpParams), int)
