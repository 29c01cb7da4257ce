"""CPU: the 3-D point-to-plane ICP's one-lane arithmetic (sfe_icp3_plane.h, through tests/host/icp3_plane_check.cpp), its
numpy restatement (tests/icp3_plane_ref.py), the inputs of the GPU tests (tests/icp3_plane_cases.py), the chain parser and the
refusals of ``pcl.ICP`` / ``store.CloudStore3``.

- icp3_plane_check against numpy: the eigenvector of random, planar-neighbourhood and near-degenerate scatter matrices within
  1e-12 per entry up to sign, every input with a relative gap (l2 - l1) / l3 >= 1e-3 between the two smallest eigenvalues (the
  error grows with 1 / gap); the 6 x 6 solve within 1e-12 relative on systems of condition <= 1e6; the pivot rule on rank 3, 4
  and 5 systems built from parallel, coplanar and two-direction normals, and on a three-wall corner; Rodrigues at theta = 0,
  1e-300, 1e-8, 1 and pi; C = 0, NaN and inf under the address and undefined-behaviour sanitizers, as a stand-alone program.
- Every ICP input of the GPU tests: the reference with its fp64 sums reversed, and with every normal moved by a float ulp,
  lands within 1e-7 of itself with equal status and iterations.  The jitter condition cannot hold for the four inputs whose
  status 5 rests on an exactly planar or collinear target (z0_target, one_wall, collinear, mixed2): the pivot rule compares a
  pivot with ITS OWN diagonal entry, so normals that are parallel to the last bit give exact zero rows (singular), while normals
  that differ by an ulp give rows that are tiny but of full relative rank (not singular, measured: status 1 after one
  step).  For those inputs the condition held instead is the fact that makes them decided by no rounding at all: every
  reference normal is exactly plus or minus one coordinate axis, the same for the whole target.
- The clouds whose normals are compared on the GPU: the share of neighbourhoods with a gap of at least 1e-3; the lattice
  tie case changes the centre normals by a right angle under ``tie_high``; the cases built for a status or a stop have it;
  point-to-plane recovers the 0.5 m slide along a wall within 1e-3 in fewer iterations than point-to-point.
- ``parse_icp_chain``, and the refusals on both routes."""
import os
import subprocess
import threading

import numpy as np
import pytest

from sonar_slam_amd import _lib as L
from sonar_slam_amd import icp_config, pcl, store

import icp3_cases as C3
import icp3_plane_cases as C
import icp3_plane_ref as R
import icp3_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "icp3_plane_check.cpp")
f32 = np.float32
EXACT_SINGULAR = ("z0_target", "one_wall", "collinear", "mixed2")


def _diff(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def _fmt(kind, v):
    return kind + " " + " ".join("%.17g" % x for x in np.ravel(v))


def _runner(exe):
    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120,
                           universal_newlines=True)
        out = r.stdout.strip().split("\n")
        assert r.returncode == 0 and out[-1] == "icp3_plane_check: ok", r.stdout[-2000:]
        assert len(out) == len(lines) + 1
        return [np.array([float(v) for v in ln.split()]) for ln in out[:-1]]
    return run


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("icp3p") / "icp3_plane_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe],
                   check=True, timeout=120)
    return _runner(exe)


def _rot(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def _some_C(rng, kind):
    """a scatter matrix V diag(l1 <= l2 <= l3) V^T with (l2 - l1) / l3 >= 1e-3"""
    l3 = 10.0 ** rng.uniform(-4, 2)
    if kind == "planar":          # a wall under noise: one eigenvalue far below the other two
        l2, l1 = l3 * rng.uniform(0.2, 1.0), l3 * 10.0 ** rng.uniform(-8, -3)
    elif kind == "near":          # the two smallest eigenvalues nearly equal: the gap at its bound
        l2 = l3 * rng.uniform(0.01, 1.0)
        l1 = l2 - l3 * 10.0 ** rng.uniform(-3, -2)
    else:
        l1, l2 = np.sort(rng.uniform(0, l3, 2))
    l1 = max(l1, 0.0)
    if (l2 - l1) / l3 < 1e-3:
        l1 = max(l2 - 1.5e-3 * l3, 0.0)
    assert (l2 - l1) / l3 >= 1e-3
    V = _rot(rng)
    C_ = V @ np.diag([l1, l2, l3]) @ V.T
    return (C_ + C_.T) / 2


def test_normal_agrees_with_numpy(check):
    rng = np.random.default_rng(21)
    Cs = [_some_C(rng, kind) for kind in ("random", "planar", "near") for _ in range(200)]
    got = check([_fmt("C", c) for c in Cs])
    worst = 0.0
    for g, c in zip(got, Cs):
        w, v = np.linalg.eigh(c)
        assert (w[1] - w[0]) / w[2] >= 0.99e-3
        n = v[:, 0]
        worst = max(worst, min(np.abs(g - n).max(), np.abs(g + n).max()))
        assert abs(np.linalg.norm(g) - 1.0) < 1e-15
    assert worst < 1e-12, worst


def _upper(A):
    return np.concatenate([A[i, i:] for i in range(6)])


def _system_of(normals, rng, n=60, cylinder=None):
    """the normal equations of n pairs whose normals are drawn from ``normals``, points anywhere in a 3 m box; with
    ``cylinder`` = (u, v, w), an orthonormal frame: points on a cylinder of radius 1.5 about w, radial normals"""
    if cylinder is None:
        N = np.asarray(normals, np.float64)[rng.integers(0, len(normals), n)]
        P = rng.uniform(-3, 3, (n, 3))
    else:
        u, v, w = cylinder
        phi = rng.uniform(0, 2 * np.pi, n)
        N = np.cos(phi)[:, None] * u + np.sin(phi)[:, None] * v
        P = 1.5 * N + rng.uniform(-2, 2, n)[:, None] * w
    Q = P + rng.normal(0, 0.05, (n, 3))
    return R.system(P, Q, N)


def test_solve_agrees_with_numpy(check):
    rng = np.random.default_rng(22)
    lines, want = [], []
    while len(lines) < 100:
        nn = rng.normal(size=(40, 3))
        A, b = _system_of(nn / np.linalg.norm(nn, axis=1)[:, None], rng)
        if np.linalg.cond(A) > 1e6:
            continue
        lines.append(_fmt("A", np.concatenate([_upper(A), b])))
        want.append(np.linalg.solve(A, b))
    for g, x in zip(check(lines), want):
        assert g[0] == 0.0
        assert np.abs(g[1:] - x).max() <= 1e-12 * np.abs(x).max(), (g[1:], x)


def test_pivot_rule_on_rank_deficient_systems(check):
    """what a surface leaves free is what the system cannot see: a plane (parallel normals) three motions, a cylinder
    (coplanar, radial normals) two, a prism (two normal directions) one, a three-wall corner none"""
    rng = np.random.default_rng(23)
    cases = []
    for V in (np.eye(3), _rot(rng)):
        cases += [("parallel", 3, dict(normals=[V[0]])), ("coplanar", 4, dict(normals=None, cylinder=(V[0], V[1], V[2]))),
                  ("two directions", 5, dict(normals=[V[0], V[1]])), ("corner", 6, dict(normals=[V[0], V[1], V[2]]))]
    lines, facts = [], []
    for name, rank, kw in cases:
        for _ in range(5):
            A, b = _system_of(rng=rng, **kw)
            s = np.linalg.svd(A, compute_uv=False)
            assert (s > 1e-9 * s[0]).sum() == rank, (name, s)          # the system has the rank it is built for
            assert R.singular(A) == (rank < 6), name
            lines.append(_fmt("A", np.concatenate([_upper(A), b])))
            facts.append((name, rank, A, b))
    for g, (name, rank, A, b) in zip(check(lines), facts):
        assert g[0] == (1.0 if rank < 6 else 0.0), (name, g)
        if rank == 6:
            assert np.abs(g[1:] - np.linalg.solve(A, b)).max() < 1e-9


def test_rodrigues(check):
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    thetas = [0.0, 1e-300, 1e-8, 1.0, np.pi]
    got = check([_fmt("R", th * axis) for th in thetas])
    for th, g in zip(thetas, got):
        Rm = g.reshape(3, 3)
        assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-15, th
        assert _diff(Rm, R.rodrigues(th * axis)) < 1e-15
        assert _diff(Rm, C3.rigid(axis, th, (0, 0, 0))[:3, :3]) < 1e-15
    assert np.array_equal(got[0].reshape(3, 3), np.eye(3))
    # the whole step: sums -> (R, t)
    rng = np.random.default_rng(24)
    A, b = _system_of(np.eye(3), rng)
    g = check([_fmt("S", np.concatenate([[60.0], _upper(A), b]))])[0]
    x = np.linalg.solve(A, b)
    assert g[0] == 0.0 and _diff(g[1:10].reshape(3, 3), R.rodrigues(x[:3])) < 1e-12 and _diff(g[10:], x[3:]) < 1e-12


def test_plane_check_under_sanitizers(tmp_path):
    """the same program with the address and undefined-behaviour sanitizers, as a stand-alone program"""
    exe = str(tmp_path / "icp3_plane_check_san")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe], check=True, timeout=180)
    rng = np.random.default_rng(25)
    lines = [_fmt("C", _some_C(rng, k)) for k in ("random", "planar", "near") for _ in range(20)]
    for v in (0.0, np.nan, np.inf, -np.inf):
        lines += [_fmt("C", np.full(9, v)), _fmt("A", np.full(27, v)), _fmt("R", np.full(3, v)), _fmt("S", np.full(28, v))]
    A, b = _system_of(np.eye(3), rng)
    lines += [_fmt("A", np.concatenate([_upper(A), b])), _fmt("R", [1e-300, 0, 0]), _fmt("R", [0, np.pi, 0])]
    got = _runner(exe)(lines)
    for ln, g in zip(lines, got):
        if ln.startswith("C "):
            assert np.isfinite(g).all() and abs(np.linalg.norm(g) - 1.0) < 1e-15          # never a NaN
        if ln.startswith(("A nan", "A inf", "A -inf", "A 0", "S nan", "S inf", "S -inf", "S 0")):
            assert g[0] == 1.0


# ---- the reference on the inputs of the GPU tests ----
@pytest.mark.parametrize("name", sorted(C.all_jobs()))
def test_gpu_input_is_stable_under_sum_order_and_normal_jitter(name):
    s, t, g, p = C.job(name)
    fin = np.isfinite(s)
    assert np.abs(s[fin]).max(initial=0.0) <= 4.0 and np.abs(t).max() <= 4.0
    nv = C.target_normals(t, p.normals_knn)
    a = C.ref(name)
    runs = [R.icp(s, t, g, p, reverse_sums=True, normals_of=nv)]
    if name in EXACT_SINGULAR:
        # (the module docstring says why an ulp of jitter cannot leave these on status 5, and what holds instead)
        assert a[0] == 5
        axis = np.abs(nv[0])
        assert sorted(axis) == [0.0, 0.0, 1.0] and np.array_equal(np.abs(nv), np.tile(axis, (len(nv), 1)))
    else:
        runs.append(R.icp(s, t, g, p, jitter_normals=5, normals_of=nv))
    for b in runs:
        assert (a[0], a[2]) == (b[0], b[2])
        if a[0] == 0:
            assert _diff(a[1], b[1]) < 1e-7
        else:
            assert np.array_equal(a[1], g, equal_nan=True) and np.array_equal(b[1], g, equal_nan=True)


def test_cases_report_what_they_are_built_for():
    for name in C.singular_jobs():
        assert C.ref(name)[0] == 5 and C.ref(name)[2] == 0, name
    assert C.ref("ns1")[0] == 5                                   # one pair: a rank-1 system
    assert C.ref("no_finite_distance")[0] == 1 and C.ref("max_dist_drops_all")[0] == 2 and C.ref("nan_in_guess")[0] == 1
    smooth = C.params().smooth_len
    assert C.ref("counter_below_smooth")[::2] == (0, 2) and 2 < smooth
    assert C.ref("counter_above_smooth")[::2] == (0, 6) and 6 > smooth
    assert C.ref("diff_at_smooth")[::2] == (0, smooth)
    it = C.ref("diff_above_smooth")[2]
    assert C.ref("diff_above_smooth")[0] == 0 and smooth + 1 < it < C.job("diff_above_smooth")[3].max_iter
    # the subset under the identity: b = 0, so the pose is the identity whatever the normals (knn = 2: segments)
    for name in ("knn2", "subset"):
        st, T, it = C.ref(name)
        assert (st, it) == (0, smooth) and _diff(T, np.eye(4)) < 1e-6, name
    for name in ("knn10", "knn16", "ns64", "ns1023", "ns1024", "ns1025", "nt4095", "nt4096", "nt4097", "nt8193"):
        assert C.ref(name)[0] == 0 and _diff(C.ref(name)[1], C3.TRUTH) < 2e-2, name
    srcs, tgts, jobs, p = C.mixed_launch()
    assert [C.ref("mixed%d" % k)[0] for k in range(len(jobs))] == [0, 5, 5, 0, 0, 0, 0, 5]
    assert len(set(C.ref("batch%d" % k)[2] for k in range(30))) > 1


def test_sliding_along_a_wall():
    s, t, g, pp, p0 = C.sliding_job()
    plane = C.ref("sliding")
    point = icp3_ref.icp(s, t, g, p0)
    print("sliding: point-to-plane", plane[0], plane[2], _diff(plane[1], np.eye(4)), "point-to-point", point[0], point[2],
          _diff(point[1], np.eye(4)))
    assert plane[0] == 0 and _diff(plane[1], np.eye(4)) < 1e-3
    assert point[0] == 0 and plane[2] < point[2]


def test_normals_clouds_have_the_gap_and_the_tie_case_depends_on_the_index():
    for n in C.NORMALS_SIZES:
        for k in C.NORMALS_KNN:
            nv, gap = C.normals_ref(n, k)
            assert np.isfinite(nv).all() and np.abs(np.linalg.norm(nv.astype(np.float64), axis=1) - 1).max() < 1e-6
            if min(k, n) >= 3:
                assert (gap >= C.GAP).mean() > 0.95, (n, k)       # what the GPU test compares
            else:
                assert (gap < C.GAP).all()                        # one or two points: nothing to compare, properties only
    cloud, k, ties = C.lattice_tie_cloud()
    lo, gap = R.normals(cloud, k, with_gap=True)
    hi = R.normals(cloud, k, tie_high=True)
    ids_lo, ids_hi = R.knn(tuple(cloud[:, a].copy() for a in range(3)), k), R.knn(tuple(cloud[:, a].copy() for a in range(3)), k, True)
    for c, chosen, refused in ties:
        assert ids_lo[c, k - 1] == chosen and ids_hi[c, k - 1] == refused and gap[c] >= C.GAP
        ang = np.arccos(min(1.0, abs(float(lo[c].astype(np.float64) @ hi[c]))))
        assert ang > 0.1, (c, ang)
    assert ties[0][1] // C.NTILE != ties[0][2] // C.NTILE and ties[1][1] // C.NTILE == ties[1][2] // C.NTILE
    cloud, k, same, run, d = C.degenerate_cloud()
    nv, gap = R.normals(cloud, k, with_gap=True)
    assert (gap[same] < C.GAP).all() and (gap[run] < C.GAP).all() and (gap[:200] >= C.GAP).mean() > 0.95
    cloud, k, bad = C.nonfinite_cloud()
    nv, gap = R.normals(cloud, k, with_gap=True)
    assert np.isfinite(nv).all() and np.array_equal(nv[bad], np.tile([1, 0, 0], (len(bad), 1)))


# ---- the parser ----
_CHAIN = """
matcher:
  KDTreeMatcher: {knn: 1, maxDist: 10.0}
outlierFilters:
  - TrimmedDistOutlierFilter: {ratio: 0.8}
errorMinimizer:
  %s
transformationCheckers:
  - CounterTransformationChecker: {maxIterationCount: 40}
"""


def test_parse_icp_chain_takes_the_3d_point_to_plane_minimiser():
    parse = icp_config.parse_icp_chain
    assert parse(_CHAIN % "PointToPlaneErrorMinimizer: {force2D: 0}").params.minimizer == 2
    assert parse(_CHAIN % "PointToPlaneErrorMinimizer").params.minimizer == 2
    assert parse(_CHAIN % "PointToPlaneErrorMinimizer: {force2D: 1}").params.minimizer == 1
    assert parse(_CHAIN % "PointToPointErrorMinimizer").params.minimizer == 0
    for bad in ("{force4DOF: 1}", "{force2D: 0, force4DOF: 1}", "{force2D: 0, sensorStdDev: 0.1}"):
        with pytest.raises(icp_config.IcpConfigError):
            parse(_CHAIN % ("PointToPlaneErrorMinimizer: " + bad))
    with pytest.raises(icp_config.IcpConfigError):                  # parse_icp_yaml keeps refusing the bare name
        icp_config.parse_icp_yaml(_CHAIN % "PointToPlaneErrorMinimizer")
    # a trailing SurfaceNormal reference stage sets normals_knn and is no device stage
    ch = parse("referenceDataPointsFilters:\n  - SurfaceNormalDataPointsFilter: {knn: 7}\n"
               + _CHAIN % "PointToPlaneErrorMinimizer: {force2D: 0}")
    assert ch.params.minimizer == 2 and ch.params.normals_knn == 7 and not ch.has_filters() and not ch.has_modules()
    assert icp_config.IcpChain.from_dict(ch.as_dict()) == ch
    p = icp_config.shipped_params(minimizer=2)
    assert p.minimizer == 2 and p.normals_knn == 10


# ---- refusals ----
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


def test_3d_point_to_plane_on_2d_clouds_reaches_no_library_call():
    c2 = np.zeros((5, 2), f32)
    e3 = np.eye(3, dtype=f32)
    j = np.array([[0, 5, 0, 5]], np.int32)
    calls = (lambda i: i.compute(c2, c2, e3), lambda i: i.compute_batch(c2, c2, [e3, e3]),
             lambda i: i.compute_pairs([c2], [c2], [e3]), lambda i: i.compute_jobs(c2, c2, j, e3.reshape(1, 9)))
    chain = icp_config.parse_icp_chain(_CHAIN % "PointToPlaneErrorMinimizer")
    for icp in (_icp(minimizer=2), _icp(chain)):
        for call in calls:
            with pytest.raises(NotImplementedError, match="force2D: 1"):
                call(icp)
        with pytest.raises(NotImplementedError, match="point-to-plane"):
            icp.getCovariance()
    with pytest.raises(NotImplementedError, match="N x 2"):
        pcl.surface_normals(c2, 10, ctx=_NoDevice())
    with pytest.raises(TypeError):
        pcl.surface_normals(np.zeros((5, 4), f32), 10, ctx=_NoDevice())
    with pytest.raises(RuntimeError, match="knn"):
        pcl.surface_normals(np.zeros((5, 3), f32), 17, ctx=_NoDevice())
    assert pcl.surface_normals(np.zeros((0, 3), f32), 10, ctx=_NoDevice()).shape == (0, 3)


def _store3_without_device():
    """a CloudStore3 whose library call is recorded, not made (``calls``)"""
    s = store.CloudStore3.__new__(store.CloudStore3)
    s.calls = []

    class _Lib(object):
        def sfe_icp3_store_compute(self, *a):
            s.calls.append(a)
            return 0

    class _Ctx(object):
        handle, lib, lock = None, _Lib(), threading.Lock()

        def _check(self, rc):
            assert rc == 0
    s.ctx, s.handle = _Ctx(), None
    return s


def test_store3_route_takes_minimiser_2_and_still_refuses_1():
    s = _store3_without_device()
    pairs, g = np.array([[0, 1]], np.int32), np.eye(4, dtype=f32)[None]
    for arg in (icp_config.shipped_params(minimizer=2), icp_config.IcpChain(icp_config.shipped_params(minimizer=2)),
                icp_config.parse_icp_chain(_CHAIN % "PointToPlaneErrorMinimizer")):
        st, T, it = s.icp(pairs, g, arg)
        assert T.shape == (1, 4, 4)
    assert len(s.calls) == 3
    for arg in (icp_config.shipped_params(minimizer=1), icp_config.IcpChain(icp_config.shipped_params(minimizer=1))):
        with pytest.raises(NotImplementedError, match="PointToPlane"):
            s.icp(pairs, g, arg)
    assert len(s.calls) == 3
    c3 = np.zeros((5, 3), f32)
    with pytest.raises(NotImplementedError, match="PointToPlane"):        # ... and pcl.ICP on N x 3, before any library call
        _icp(minimizer=1).compute(c3, c3, np.eye(4, dtype=f32))


def test_header_declares_normals3_and_the_library_exports_it():
    hdr = open(os.path.join(ROOT, "include", "sonarfe.h")).read()
    assert "int sfe_normals3(sfe_ctx *ctx, const float *pts, int n, int knn, float *normals_out);" in hdr
    lib = L.load_library()
    assert "sfe_normals3" in L.SIGNATURES and hasattr(lib, "sfe_normals3")
    assert lib.sfe_normals3(None, None, 0, 10, None) < 0               # no context: SFE_ERR_ARG before anything else
