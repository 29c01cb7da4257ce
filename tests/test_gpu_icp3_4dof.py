"""GPU: the 4-DoF point-to-plane minimiser of the 3-D ICP -- ``pcl.ICP`` with ``shipped_params(minimizer=3)`` or a ``dims=3``
chain that says ``PointToPlaneErrorMinimizer {force4DOF: 1}`` (icp3_job_kernel<3, 0> and <3, 1>, sfe_icp3.hip) -- against the
numpy restatement of its rule (tests/icp3_4dof_ref.py).  The inputs are built in tests/icp3_4dof_cases.py;
tests/test_icp3_4dof_host.py holds every one of them to its conditions on the CPU (stable under the order of the sums and
under an ulp of jitter on the normals; statuses, stops and ranks as built).

The bar is the one of tests/test_gpu_icp3_plane.py: status and iterations equal, T within 1e-6 per entry, T = the guess on a
failure.  Shapes (1024 threads per job, two queries per lane and pass, a target tile of 4096 points in LDS): source counts
1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 2049 on 300 targets; target counts 3, 4095, 4096, 4097 under 200 sources;
normals_knn 2, 10, 16.  A guess that rotates about z only leaves entries (0,2), (1,2), (2,0), (2,1) of T exactly 0 and (2,2)
exactly 1, on a scene rolled by 2 degrees that the 6-DoF minimiser follows; status 5 on a z = 0 target, one wall, upright
walls (n_z = 0) and a single source point, status 2 on an empty keep set; Counter, Differential and NaN stops; one launch of
8 jobs of different sizes with failing ones among them; 30 guesses; the store route; a parsed dims = 3 chain with an octree
stage, MedianDist and Bound, bit for bit ICP on the clouds filtered beforehand; the refusals."""
import numpy as np
import pytest

from sonar_slam_amd import _lib as L
from sonar_slam_amd import icp_config, pcl, store
from sonar_slam_amd.pipeline import ScanMatchBatch

import icp3_4dof_cases as C
import icp3_4dof_ref as R
import icp3_plane_ref as RP

pytestmark = pytest.mark.gpu

TOL_TIGHT = 1e-6        # tests/test_gpu_icp3_plane.py's bound on the pose against the reference
ERR_ARG = r"libsonarfe error %d:" % L.SFE_ERR_ARG
f32 = np.float32


def _icp(ctx, p):
    icp = pcl.ICP(ctx=ctx)
    icp.setParams(p)
    return icp


def _diff(Ta, Tb):
    return float(np.abs(np.asarray(Ta, np.float64) - np.asarray(Tb, np.float64)).max())


def _hold(got, want, guess, info):
    st, T, it = got
    print(info, "status", int(st), want[0], "iterations", int(it), want[2], "diff",
          _diff(T, want[1]) if want[0] == 0 else None)
    assert (int(st), int(it)) == (want[0], want[2]), info
    assert T.shape == (4, 4) and T.dtype == np.float32
    if want[0] == 0:
        assert _diff(T, want[1]) < TOL_TIGHT, (info, _diff(T, want[1]))
    else:
        assert np.array_equal(T, guess, equal_nan=True), info


def _run(ctx, name):
    s, t, g, p = C.job(name)
    st, T, it = _icp(ctx, p).compute_jobs(s, t, np.array([[0, len(s), 0, len(t)]], np.int32), g.reshape(1, 16))
    _hold((st[0], T[0], it[0]), C.ref(name), g, name)
    return int(st[0]), T[0], int(it[0])


def _yaw_only(T):
    """the rotation block has the z row and the z column of a rotation about z, to the bit"""
    return bool(np.array_equal(T[2, :3], [0, 0, 1]) and np.array_equal(T[:3, 2], [0, 0, 1]))


# ---- parity ----
@pytest.mark.parametrize("ns", C.SOURCE_COUNTS)
def test_source_counts(ctx, ns):
    st, T, it = _run(ctx, "ns%d" % ns)
    assert st == (5 if ns < 4 else 0)                                 # fewer pairs than unknowns


@pytest.mark.parametrize("nt", C.TARGET_COUNTS)
def test_target_counts(ctx, nt):
    st, T, it = _run(ctx, "nt%d" % nt)
    assert st == (5 if nt == 3 else 0)                                # three target points: one plane


@pytest.mark.parametrize("knn", C.KNN)
def test_normals_knn(ctx, knn):
    st, T, it = _run(ctx, "knn%d" % knn)
    assert st == 0
    if knn == 2:      # the subset under the identity guess: b = 0, gamma = 0
        assert _diff(T, np.eye(4)) < TOL_TIGHT
    else:
        assert _diff(T, C.TRUTH) < 2e-2
    s, t, g, p = C.job("knn%d" % knn)
    msg, T1 = _icp(ctx, p).compute(s, t, g)
    assert msg == "success" and np.array_equal(T1, T)


# ---- the step has yaw and translation only ----
def test_a_yaw_only_guess_gives_an_exact_yaw_only_pose(ctx):
    # (tests/test_icp3_4dof_host.py asserts the same of the two references first)
    s, t, g, p4, p6 = C.roll_job()
    assert _yaw_only(g)
    st, T4, it = _run(ctx, "roll")
    assert st == 0 and it >= 1 and _yaw_only(T4)
    msg6, T6 = _icp(ctx, p6).compute(s, t, g)
    print("roll: 4-DoF", it, T4[2, :3], "6-DoF", msg6, T6[2, :3])
    assert msg6 == "success" and not _yaw_only(T6)
    assert abs(float(T6[2, 1])) > 0.02 and abs(float(T6[1, 2])) > 0.02        # sin(2 degrees) = 0.035: it follows the roll
    # ... after every number of iterations, not only at the fixed point
    for k in (1, 2, 3):
        msgs, Tk, itk = _icp(ctx, C.params(max_iter=k)).compute_batch(s, t, [g])
        assert msgs == ["success"] and itk[0] == k and _yaw_only(Tk[0])


# ---- rank rules ----
@pytest.mark.parametrize("name", sorted(C.RANK_STATUS))
def test_rank_rules(ctx, name):
    st, T, it = _run(ctx, name)
    assert (st, it) == (C.RANK_STATUS[name], 0)
    s, t, g, p = C.job(name)
    msg, T1 = _icp(ctx, p).compute(s, t, g)
    assert msg == L.ICP_STATUS_MESSAGES[st] and np.array_equal(T1, g)


# ---- statuses and stops ----
@pytest.mark.parametrize("name", sorted(C.status_jobs()))
def test_statuses_and_stops(ctx, name):
    st, T, it = _run(ctx, name)
    s, t, g, p = C.job(name)
    msg, T1 = _icp(ctx, p).compute(s, t, g)
    assert msg == L.ICP_STATUS_MESSAGES[st] and np.array_equal(T1, T, equal_nan=True)


# ---- launches ----
def _tables(srcs, tgts, jobs):
    so = np.concatenate([[0], np.cumsum([len(s) for s in srcs])])
    to = np.concatenate([[0], np.cumsum([len(t) for t in tgts])])
    j4 = np.array([(so[a], len(srcs[a]), to[b], len(tgts[b])) for a, b, g in jobs], np.int32)
    return j4, np.stack([g for a, b, g in jobs])


def test_one_launch_mixing_jobs(ctx):
    srcs, tgts, jobs, p = C.mixed_launch()
    icp = _icp(ctx, p)
    single = [icp.compute_batch(srcs[a], tgts[b], [g]) for a, b, g in jobs]
    for k, (a, b, g) in enumerate(jobs):
        msgs, T, it = single[k]
        want = C.ref("mixed%d" % k)
        assert msgs[0] == L.ICP_STATUS_MESSAGES[want[0]]
        _hold((want[0], T[0], it[0]), want, g, "mixed%d" % k)
    assert [C.ref("mixed%d" % k)[0] for k in range(len(jobs))] == C.MIXED_STATUS
    msgs, T, it = icp.compute_pairs([srcs[a] for a, b, g in jobs], [tgts[b] for a, b, g in jobs], [g for a, b, g in jobs])
    for k in range(len(jobs)):
        assert msgs[k] == single[k][0][0] and np.array_equal(T[k], single[k][1][0]) and it[k] == single[k][2][0], k
    j4, gs = _tables(srcs, tgts, jobs)
    st, T2, it2 = icp.compute_jobs(np.concatenate(srcs), np.concatenate(tgts), j4, gs.reshape(-1, 16))
    assert st.tolist() == C.MIXED_STATUS
    for k in range(len(jobs)):
        assert np.array_equal(T2[k], single[k][1][0]) and it2[k] == single[k][2][0], k


def test_compute_batch_of_30_guesses(ctx):
    s, t, _ = C.batch_pair()
    gs = C.batch_guesses()
    icp = _icp(ctx, C.params())
    msgs, T, it = icp.compute_batch(s, t, gs)
    assert T.shape == (30, 4, 4)
    for k, g in enumerate(gs):
        want = C.ref("batch%d" % k)
        assert msgs[k] == L.ICP_STATUS_MESSAGES[want[0]]
        _hold((want[0], T[k], it[k]), want, g, "batch%d" % k)
        assert _yaw_only(g) and _yaw_only(T[k])                      # yaw-only guesses: yaw-only poses, to the bit
    for k in (0, 17, 29):                                            # the normals taken once for 30 jobs, or for this one
        msg, T1 = icp.compute(s, t, gs[k])
        assert msg == msgs[k] and np.array_equal(T1, T[k]), k
    assert len(set(int(i) for i in it)) > 1


def test_store_route_is_the_host_pointer_call(ctx):
    srcs, tgts, jobs, p = C.mixed_launch()
    clouds = srcs + tgts
    st3 = store.CloudStore3(ctx, capacity_points=sum(len(c) for c in clouds), max_clouds=len(clouds))
    try:
        h = [st3.put(c) for c in clouds]
        pairs = np.array([(h[a], h[len(srcs) + b]) for a, b, g in jobs], np.int32)
        j4, gs = _tables(srcs, tgts, jobs)
        st2, T2, it2 = _icp(ctx, p).compute_jobs(np.concatenate(srcs), np.concatenate(tgts), j4, gs.reshape(-1, 16))
        for arg in (p, icp_config.IcpChain(p), icp_config.IcpChain(p, dims=3)):
            st, T, it = st3.icp(pairs, gs, arg)
            assert np.array_equal(st, st2) and np.array_equal(it, it2)
            assert np.array_equal(T.view(np.uint32), T2.view(np.uint32))
        assert st2.tolist() == C.MIXED_STATUS
    finally:
        st3.close()


# ---- a chain written for three dimensions: <3, 1> behind its data-point filters ----
CHAIN_4DOF = """
referenceDataPointsFilters:
  - OctreeGridDataPointsFilter: {maxSizeByNode: 0.2, samplingMethod: 3}
matcher:
  KDTreeMatcher: {knn: 1, maxDist: 10.0}
outlierFilters:
  - MaxDistOutlierFilter: {maxDist: 3.0}
  - TrimmedDistOutlierFilter: {ratio: 0.8}
  - MedianDistOutlierFilter: {factor: 2.5}
errorMinimizer:
  PointToPlaneErrorMinimizer: {force2D: 0, force4DOF: 1}
transformationCheckers:
  - CounterTransformationChecker: {maxIterationCount: 40}
  - DifferentialTransformationChecker: {minDiffRotErr: 0.01, minDiffTransErr: 0.1, smoothLength: 4}
  - BoundTransformationChecker: {maxRotationNorm: 1.0, maxTranslationNorm: 5.0}
"""


def test_a_dims3_chain_is_icp_on_the_clouds_filtered_beforehand(ctx, tmp_path):
    path = tmp_path / "icp4dof.yaml"
    path.write_text(CHAIN_4DOF)
    icp = pcl.ICP(ctx)
    icp.loadFromYaml(str(path), dims=3)
    chain = icp.chain
    assert chain.dims == 3 and chain.params.minimizer == 3 and chain.has_filters()
    assert chain.outliers.use_median and chain.outliers.use_bound and chain.outliers.bound_order == 3
    s, t, _ = C.batch_pair()
    gs = C.batch_guesses()[:6]
    msgs, T, it = icp.compute_batch(s, t, gs)
    assert msgs == ["success"] * len(gs)
    ft = pcl.downsample(t, 0.2, ctx=ctx)
    assert 100 < len(ft) < len(t)
    pre = pcl.ICP(ctx)
    pre.setChain(icp_config.IcpChain(chain.params, outliers=chain.outliers, dims=3))          # the modules, no stage
    m2, T2, it2 = pre.compute_batch(s, ft, gs)
    assert m2 == msgs and np.array_equal(it, it2) and np.array_equal(T.view(np.uint32), T2.view(np.uint32))
    # ... and the store runs the same chain to the same bits
    st3 = store.CloudStore3(ctx, capacity_points=len(s) + len(t), max_clouds=2)
    try:
        hs, ht = st3.put(s), st3.put(t)
        st, T3, it3 = st3.icp(np.array([[hs, ht]] * len(gs), np.int32), np.stack(gs), chain)
        assert not st.any() and np.array_equal(it3, it) and np.array_equal(T3.view(np.uint32), T.view(np.uint32))
    finally:
        st3.close()
    # against the reference with the chain's modules, on the filtered target and its own normals
    nv = RP.normals(ft, chain.params.normals_knn, centre=True)
    for k in (0, len(gs) - 1):
        want = R.icp(s, ft, gs[k], chain.params, chain.outliers, normals_of=nv)
        _hold((0, T[k], it[k]), want, gs[k], "chain guess %d" % k)
    # a Bound that the first step leaves: status 9, T = the guess
    tight = icp_config.IcpChain.from_dict(chain.as_dict())
    tight.outliers.max_translation_norm = 1e-4
    tight.outliers.max_rotation_norm = 1e-5
    icp.setChain(tight)
    msgs, T9, it9 = icp.compute_batch(s, t, gs[:2])
    for k in range(2):
        want = R.icp(s, ft, gs[k], tight.params, tight.outliers, normals_of=nv)
        assert want[0] == 9 and msgs[k] == L.ICP_STATUS_MESSAGES[9]
        _hold((9, T9[k], it9[k]), want, gs[k], "bound guess %d" % k)


# ---- refusals ----
def test_refusals_reach_no_kernel(ctx):
    c3, c2 = np.zeros((5, 3), f32), np.zeros((5, 2), f32)
    j = np.array([[0, 5, 0, 5]], np.int32)
    p3 = icp_config.shipped_params(minimizer=3)
    e3 = np.eye(3, dtype=f32)
    # N x 2 clouds: refused in Python, whichever way the chain was installed
    by_chain = pcl.ICP(ctx=ctx)
    by_chain.setChain(icp_config.parse_icp_chain(CHAIN_4DOF, dims=3))
    for icp in (_icp(ctx, p3), by_chain):
        for call in (lambda i: i.compute(c2, c2, e3), lambda i: i.compute_batch(c2, c2, [e3]),
                     lambda i: i.compute_pairs([c2], [c2], [e3]), lambda i: i.compute_jobs(c2, c2, j, e3.reshape(1, 9))):
            with pytest.raises(NotImplementedError, match="force4DOF"):
                call(icp)
    # normals_knn outside [2, 16]
    for knn in (1, 17):
        with pytest.raises(L.SonarFEError, match=ERR_ARG):
            _icp(ctx, icp_config.shipped_params(minimizer=3, normals_knn=knn)).compute(c3, c3, np.eye(4, dtype=f32))
    # minimizer 1 on N x 3 keeps its words, and a value nobody knows is refused
    for m in (1, 4):
        with pytest.raises(L.SonarFEError, match="point-to-point"):
            _icp(ctx, icp_config.shipped_params(minimizer=m))._call3(
                ctx, c3, c3, j, np.eye(4, dtype=f32).reshape(1, 16), np.zeros((1, 4, 4), f32), np.zeros(1, np.int32),
                np.zeros(1, np.int32))
    # every 2-D entry point refuses minimizer 3
    g9 = e3.reshape(1, 9)
    off = np.array([0, 5], np.int32)
    T, st, it = np.zeros((1, 3, 3), f32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    stage = L.IcpDpf(kind=L.DPF_MAX_DIST, dim=-1, remove_inside=0)
    stage.f[0] = 20.0
    chains = [icp_config.IcpChain(p3), icp_config.IcpChain(p3, reading=[stage]), icp_config.IcpChain(p3, reference=[stage]),
              icp_config.IcpChain(p3, outliers=L.IcpOutliers(use_median=1, median_factor=3.0))]
    for chain in chains:
        icp2 = pcl.ICP(ctx=ctx)
        icp2.setChain(chain)
        for shape, clouds in (("guesses", (L.ptr(c2, L.C.c_float), 5, L.ptr(c2, L.C.c_float), 5)),
                              ("pairs", (L.ptr(c2, L.C.c_float), L.ptr(off, L.C.c_int32), L.ptr(c2, L.C.c_float),
                                         L.ptr(off, L.C.c_int32))),
                              ("jobs", (L.ptr(c2, L.C.c_float), 5, L.ptr(c2, L.C.c_float), 5, L.ptr(j, L.C.c_int32)))):
            with pytest.raises(L.SonarFEError, match=ERR_ARG):
                icp2._call(ctx, shape, clouds, g9, 1, T, st, it)
    with ctx.lock:                                                   # sfe_icp_compute: the single-pair entry point
        rc = ctx.lib.sfe_icp_compute(ctx.handle, L.C.byref(p3), L.ptr(c2, L.C.c_float), 5, L.ptr(c2, L.C.c_float), 5,
                                     L.ptr(g9, L.C.c_float), L.ptr(T, L.C.c_float), None)
    assert rc == L.SFE_ERR_ARG
    s2 = store.CloudStore(ctx, capacity_points=64, max_clouds=4)
    try:
        h = s2.put(np.zeros((5, 2), f32))
        for chain in (p3, chains[1], chains[3]):
            with pytest.raises(L.SonarFEError, match=ERR_ARG):
                s2.icp(chain, np.array([[h, h]], np.int32), g9.reshape(1, 3, 3))
    finally:
        s2.close()
    b = ScanMatchBatch(ctx, p3, [c2], [c2], [(0, 0)], [np.eye(3, dtype=f32)])          # sfe_icp_jobs_dev
    try:
        with pytest.raises(L.SonarFEError, match=ERR_ARG):
            b.run()
    finally:
        b.free()
    assert not st.any() and not T.any()
