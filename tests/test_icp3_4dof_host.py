"""CPU: the 4-DoF point-to-plane step of the 3-D ICP (``minimizer == 3``, libpointmatcher's ``force4DOF: 1``) -- its one-lane
arithmetic (sfe_icp3_plane.h: icp3p_chol4, icp3p_rot_z, icp3p_solve4, through tests/host/icp3_4dof_check.cpp), its numpy
restatement (tests/icp3_4dof_ref.py), the inputs of the GPU tests (tests/icp3_4dof_cases.py), the chain parser and the
refusals of ``pcl.ICP``.

- icp3_4dof_check against numpy: the 4 x 4 solve within 1e-12 per entry (relative to the largest entry of x, the bar of
  tests/test_icp3_plane_host.py) on systems of condition <= 1e6; the pivot rule on systems of rank 1, 2 and 3 built from
  parallel normals, normals with n_z = 0 and points that give no yaw information, and on a three-wall corner (rank 4); the
  rotation about z exact at 0 and within 1e-15 at +-pi/2 and +-pi; zero, NaN and infinite input under the address and
  undefined-behaviour sanitizers, as a stand-alone program.
- Every ICP input of the GPU tests: the reference with its fp64 sums reversed, and with every normal moved by a float ulp,
  lands within 1e-7 of itself with equal status and iterations.  As tests/test_icp3_plane_host.py says for the 6-DoF inputs,
  the jitter condition cannot hold where status 5 rests on exact zeros (z0_target, one_wall, upright_walls and the launch's job
  on the z = 0 target): the pivot rule compares a pivot with its own diagonal entry, so a diagonal entry that jitter lifts
  from 0 to 1e-14 is of full relative rank.  For those the condition held instead is what makes them decided by no rounding
  at all: every reference normal is exactly plus or minus a coordinate axis.
- The cases built for a status, a stop or a rank have it; the rolled scene leaves a roll in the 6-DoF reference's T and none
  in the 4-DoF one's.
- ``parse_icp_chain``: the accept and refuse table of ``force4DOF``; the refusals on N x 2 clouds."""
import os
import subprocess

import numpy as np
import pytest

from sonar_slam_amd import icp_config, pcl

import icp3_4dof_cases as C
import icp3_4dof_ref as R
import icp3_cases as C3
import icp3_plane_ref as RP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "icp3_4dof_check.cpp")
f32 = np.float32
EXACT_SINGULAR = C.EXACT_SINGULAR + ("mixed2",)


def _diff(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def _fmt(kind, v):
    return kind + " " + " ".join("%.17g" % x for x in np.ravel(v))


def _runner(exe):
    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120,
                           universal_newlines=True)
        out = r.stdout.strip().split("\n")
        assert r.returncode == 0 and out[-1] == "icp3_4dof_check: ok", r.stdout[-2000:]
        assert len(out) == len(lines) + 1
        return [np.array([float(v) for v in ln.split()]) for ln in out[:-1]]
    return run


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("icp3p4") / "icp3_4dof_check")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe],
                   check=True, timeout=120)
    return _runner(exe)


def _upper(A):
    return np.concatenate([A[i, i:] for i in range(4)])


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1)[..., None]


def _system_of(kind, rng, n=60):
    """the 4 x 4 normal equations of n pairs in a 3 m box, by what the surface leaves free"""
    P = rng.uniform(-3, 3, (n, 3))
    if kind == "generic":
        N = _unit(rng.normal(size=(n, 3)))
    elif kind == "corner":                        # three walls: every motion is seen
        N = np.eye(3)[rng.integers(0, 3, n)]
    elif kind == "parallel_z":                    # a floor: F = (0, 0, 0, 1), only t_z is seen (rank 1)
        N = np.tile([0.0, 0.0, 1.0], (n, 1))
    elif kind == "parallel":                      # one wall with a generic normal: F = (c, n), two directions (rank 2)
        N = np.tile(_unit([0.3, -0.5, 0.8]), (n, 1))
    elif kind == "upright":                       # upright walls of every heading: n_z = 0, t_z is free (rank 3)
        phi = rng.uniform(0, 2 * np.pi, n)
        N = np.stack([np.cos(phi), np.sin(phi), 0 * phi], 1)
    elif kind == "no_yaw":                        # points in the planes y = 0 and x = 0 with normals in their plane: (n_x, n_y)
        in_x = rng.random(n) < 0.5                # along (p_x, p_y), so c = 0 to the bit and the yaw is not seen (rank 3)
        P[:, 0], P[:, 1] = np.where(in_x, P[:, 0], 0.0), np.where(in_x, 0.0, P[:, 1])
        N = _unit(rng.normal(size=(n, 3)))
        N[:, 0], N[:, 1] = np.where(in_x, N[:, 0], 0.0), np.where(in_x, 0.0, N[:, 1])
        N = _unit(N)
    Q = P + rng.normal(0, 0.05, (n, 3))
    return R.system(P, Q, N)


def test_solve_agrees_with_numpy(check):
    rng = np.random.default_rng(31)
    lines, want = [], []
    while len(lines) < 100:
        A, b = _system_of("generic", rng)
        if np.linalg.cond(A) > 1e6:
            continue
        lines.append(_fmt("A", np.concatenate([_upper(A), b])))
        want.append(np.linalg.solve(A, b))
    for g, x in zip(check(lines), want):
        assert g[0] == 0.0
        assert np.abs(g[1:] - x).max() <= 1e-12 * np.abs(x).max(), (g[1:], x)


def test_pivot_rule_on_rank_deficient_systems(check):
    rng = np.random.default_rng(32)
    cases = [("parallel_z", 1), ("parallel", 2), ("upright", 3), ("no_yaw", 3), ("corner", 4), ("generic", 4)]
    lines, facts = [], []
    for kind, rank in cases:
        for _ in range(5):
            A, b = _system_of(kind, rng)
            s = np.linalg.svd(A, compute_uv=False)
            assert (s > 1e-9 * s[0]).sum() == rank, (kind, s)          # the system has the rank it is built for
            assert R.singular(A) == (rank < 4), kind
            lines.append(_fmt("A", np.concatenate([_upper(A), b])))
            facts.append((kind, rank, A, b))
    for g, (kind, rank, A, b) in zip(check(lines), facts):
        assert g[0] == (1.0 if rank < 4 else 0.0), (kind, g)
        if rank == 4:
            assert np.abs(g[1:] - np.linalg.solve(A, b)).max() < 1e-9


def test_rotation_about_z_and_the_whole_step(check):
    gammas = [0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi, 1e-300, 1e-8, 1.0]
    got = check([_fmt("Z", [g]) for g in gammas])
    assert np.array_equal(got[0].reshape(3, 3), np.eye(3))                       # exact at 0
    for g, r in zip(gammas, got):
        Rm = r.reshape(3, 3)
        assert np.array_equal(Rm[2], [0, 0, 1]) and np.array_equal(Rm[:, 2], [0, 0, 1])
        assert _diff(Rm, R.rot_z(g)) < 1e-15 and _diff(Rm, C3.rigid((0, 0, 1), g, (0, 0, 0))[:3, :3]) < 1e-15
    for g, want in ((np.pi / 2, [[0, -1], [1, 0]]), (-np.pi / 2, [[0, 1], [-1, 0]]), (np.pi, [[-1, 0], [0, -1]]),
                    (-np.pi, [[-1, 0], [0, -1]])):
        assert _diff(got[gammas.index(g)].reshape(3, 3)[:2, :2], want) < 1e-15
    # the whole step: sums -> (R, t)
    rng = np.random.default_rng(33)
    A, b = _system_of("corner", rng)
    g = check([_fmt("S", np.concatenate([[60.0], _upper(A), b]))])[0]
    x = np.linalg.solve(A, b)
    assert g[0] == 0.0 and _diff(g[1:10].reshape(3, 3), R.rot_z(x[0])) < 1e-12 and _diff(g[10:], x[1:]) < 1e-12
    Rs, ts = R.step(A, b)
    assert _diff(g[1:10].reshape(3, 3), Rs) < 1e-12 and _diff(g[10:], ts) < 1e-12


def test_4dof_check_under_sanitizers(tmp_path):
    """the same program with the address and undefined-behaviour sanitizers, as a stand-alone program"""
    exe = str(tmp_path / "icp3_4dof_check_san")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe], check=True, timeout=180)
    rng = np.random.default_rng(34)
    lines = []
    for kind in ("generic", "corner", "parallel_z", "parallel", "upright", "no_yaw"):
        for _ in range(10):
            A, b = _system_of(kind, rng)
            lines += [_fmt("A", np.concatenate([_upper(A), b])), _fmt("S", np.concatenate([[60.0], _upper(A), b]))]
    for v in (0.0, np.nan, np.inf, -np.inf):
        lines += [_fmt("A", np.full(14, v)), _fmt("Z", [v]), _fmt("S", np.full(15, v))]
    lines += [_fmt("Z", [1e-300]), _fmt("Z", [np.pi]), _fmt("Z", [1e300])]
    got = _runner(exe)(lines)
    for ln, g in zip(lines, got):
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
        assert all(sorted(row) == [0.0, 0.0, 1.0] for row in np.abs(nv))
    else:
        runs.append(R.icp(s, t, g, p, jitter_normals=5, normals_of=nv))
    for b in runs:
        assert (a[0], a[2]) == (b[0], b[2])
        if a[0] == 0:
            assert _diff(a[1], b[1]) < 1e-7
        else:
            assert np.array_equal(a[1], g, equal_nan=True) and np.array_equal(b[1], g, equal_nan=True)


def test_cases_report_what_they_are_built_for():
    for name, status in C.RANK_STATUS.items():
        assert C.ref(name)[0] == status and C.ref(name)[2] == 0, name
    # the exact targets have the normals their rank rests on: all +-z, all +-x, all +-x or +-y
    nz = np.abs(C.target_normals(C.job("z0_target")[1], 10))
    nw = np.abs(C.target_normals(C.job("one_wall")[1], 10))
    nu = np.abs(C.target_normals(C.job("upright_walls")[1], C.UPRIGHT_KNN))
    assert (nz == [0, 0, 1]).all() and (nw == [1, 0, 0]).all()
    assert (nu[:, 2] == 0).all() and (nu[:, 0] == 1).any() and (nu[:, 1] == 1).any()
    for ns in (1, 2, 3):                                          # fewer pairs than unknowns
        assert C.ref("ns%d" % ns)[0] == 5, ns
    assert C.ref("nt3")[0] == 5                                   # three target points: one plane, parallel normals
    assert C.ref("no_finite_distance")[0] == 1 and C.ref("max_dist_drops_all")[0] == 2 and C.ref("nan_in_guess")[0] == 1
    smooth = C.params().smooth_len
    assert C.ref("counter_below_smooth")[::2] == (0, 2) and 2 < smooth
    assert C.ref("counter_above_smooth")[::2] == (0, 6) and 6 > smooth
    assert C.ref("diff_at_smooth")[::2] == (0, smooth)
    it = C.ref("diff_above_smooth")[2]
    assert C.ref("diff_above_smooth")[0] == 0 and smooth + 1 < it < C.job("diff_above_smooth")[3].max_iter
    st, T, it = C.ref("knn2")                                     # the subset under the identity: b = 0, gamma = 0
    assert (st, it) == (0, smooth) and _diff(T, np.eye(4)) < 1e-6
    names = ["knn10", "knn16"] + ["ns%d" % n for n in C.SOURCE_COUNTS[3:]] + ["nt%d" % n for n in C.TARGET_COUNTS[1:]]
    for name in names:
        assert C.ref(name)[0] == 0 and _diff(C.ref(name)[1], C.TRUTH) < 2e-2, name
    srcs, tgts, jobs, p = C.mixed_launch()
    assert [C.ref("mixed%d" % k)[0] for k in range(len(jobs))] == C.MIXED_STATUS
    assert len(set(len(srcs[a]) for a, b, g in jobs)) > 1 and len(set(len(tgts[b]) for a, b, g in jobs)) > 1
    assert all(C.ref("batch%d" % k)[0] == 0 for k in range(30))
    assert len(set(C.ref("batch%d" % k)[2] for k in range(30))) > 1


def test_the_rolled_scene_keeps_a_4dof_pose_free_of_roll_and_pitch():
    s, t, g, p4, p6 = C.roll_job()
    assert np.array_equal(g[2, :3], [0, 0, 1]) and np.array_equal(g[:3, 2], [0, 0, 1])      # the guess rotates about z only
    st4, T4, it4 = C.ref("roll")
    st6, T6, it6 = RP.icp(s, t, g, p6, normals_of=C.target_normals(t, p6.normals_knn))
    print("roll: 4-DoF", st4, it4, T4[2, :3], "6-DoF", st6, it6, T6[2, :3])
    assert st4 == 0 and st6 == 0
    assert np.array_equal(T4[2, :3], [0, 0, 1]) and np.array_equal(T4[:3, 2], [0, 0, 1])
    assert abs(float(T6[2, 1])) > 0.02 and abs(float(T6[1, 2])) > 0.02                      # sin(2 degrees) = 0.035


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
_P2PL = "PointToPlaneErrorMinimizer: "


def test_parse_icp_chain_reads_force4dof_in_a_3d_chain_only():
    parse = icp_config.parse_icp_chain
    for text in ("{force4DOF: 1}", "{force2D: 0, force4DOF: 1}", "{force4DOF: 1, force2D: 0}"):
        ch = parse(_CHAIN % (_P2PL + text), dims=3)
        assert ch.params.minimizer == 3 and ch.dims == 3 and ch.params.normals_knn == 10
        assert icp_config.IcpChain.from_dict(ch.as_dict()) == ch
        assert icp_config.IcpChain.from_dict(ch.as_dict()).params.minimizer == 3
    for text in ("{force4DOF: 0}", "{force2D: 0, force4DOF: 0}", "{force2D: 0}"):
        assert parse(_CHAIN % (_P2PL + text), dims=3).params.minimizer == 2
    assert parse(_CHAIN % "PointToPlaneErrorMinimizer", dims=3).params.minimizer == 2
    assert parse(_CHAIN % (_P2PL + "{force2D: 1}"), dims=3).params.minimizer == 1
    for bad in ("{force2D: 1, force4DOF: 1}", "{force4DOF: 1, sensorStdDev: 0.1}", "{force4DOF: 1, force3DOF: 1}"):
        with pytest.raises(icp_config.IcpConfigError):
            parse(_CHAIN % (_P2PL + bad), dims=3)
    # a chain written for two dimensions (the default) refuses the parameter, whatever its value; parse_icp_yaml too
    for bad in ("{force4DOF: 1}", "{force2D: 0, force4DOF: 1}", "{force4DOF: 0}"):
        with pytest.raises(icp_config.IcpConfigError):
            parse(_CHAIN % (_P2PL + bad))
        with pytest.raises(icp_config.IcpConfigError):
            parse(_CHAIN % (_P2PL + bad), dims=2)
        with pytest.raises(icp_config.IcpConfigError):
            icp_config.parse_icp_yaml(_CHAIN % (_P2PL + bad))
    # a trailing SurfaceNormal reference stage sets normals_knn and is no device stage
    ch = parse("referenceDataPointsFilters:\n  - SurfaceNormalDataPointsFilter: {knn: 7}\n" + _CHAIN % (_P2PL + "{force4DOF: 1}"),
               dims=3)
    assert ch.params.minimizer == 3 and ch.params.normals_knn == 7 and not ch.has_filters() and not ch.has_modules()
    assert icp_config.IcpChain.from_dict(ch.as_dict()) == ch
    p = icp_config.shipped_params(minimizer=3)
    assert p.minimizer == 3 and p.normals_knn == icp_config.shipped_params(minimizer=2).normals_knn == 10


def test_load_from_yaml_with_dims_3(tmp_path):
    path = tmp_path / "icp4dof.yaml"
    path.write_text(_CHAIN % (_P2PL + "{force4DOF: 1}"))
    icp = pcl.ICP(ctx=_NoDevice())
    icp.loadFromYaml(str(path), dims=3)
    assert icp.params.minimizer == 3 and icp.chain.dims == 3
    with pytest.raises(icp_config.IcpConfigError, match="force4DOF"):
        pcl.ICP(ctx=_NoDevice()).loadFromYaml(str(path))              # dims = 2: refused


# ---- refusals ----
class _NoDevice(object):
    """a context that fails the test if a refused call reaches the library"""
    def __getattr__(self, name):
        raise AssertionError("the call reached the device context (%s)" % name)


def test_4dof_on_2d_clouds_reaches_no_library_call():
    c2 = np.zeros((5, 2), f32)
    e3 = np.eye(3, dtype=f32)
    j = np.array([[0, 5, 0, 5]], np.int32)
    calls = (lambda i: i.compute(c2, c2, e3), lambda i: i.compute_batch(c2, c2, [e3, e3]),
             lambda i: i.compute_pairs([c2], [c2], [e3]), lambda i: i.compute_jobs(c2, c2, j, e3.reshape(1, 9)))
    a, b = pcl.ICP(ctx=_NoDevice()), pcl.ICP(ctx=_NoDevice())
    a.setParams(icp_config.shipped_params(minimizer=3))
    b.setChain(icp_config.parse_icp_chain(_CHAIN % (_P2PL + "{force4DOF: 1}"), dims=3))
    for icp in (a, b):
        for call in calls:
            with pytest.raises(NotImplementedError, match="force4DOF"):
                call(icp)
        with pytest.raises(NotImplementedError, match="point-to-plane"):
            icp.getCovariance()
