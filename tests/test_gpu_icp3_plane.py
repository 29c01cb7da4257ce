"""GPU: the 3-D point-to-plane chain -- ``pcl.surface_normals`` (normals3_kernel) and ``pcl.ICP`` with
``shipped_params(minimizer=2)`` (icp3_job_kernel<2>, sfe_icp3.hip) -- against the numpy restatement of its rules
(tests/icp3_plane_ref.py).  The inputs are built in tests/icp3_plane_cases.py; tests/test_icp3_plane_host.py holds every one of
them to its conditions on the CPU (stable under the order of the sums and under an ulp of jitter on the normals, eigen-gaps,
ties, statuses, stops).

Normals: per component within 2^-23 of the reference up to sign (one float ulp below magnitude 1: what rounding an fp64 vector
known to 1e-12 can move), wherever the neighbourhood's relative eigen-gap is at least 1e-3; everywhere: finite and of unit
length within 1e-6.  Sizes 1, 2, 3, 255, 256, 257 (the lanes of a workgroup), 2047, 2048, 2049, 4097 (its LDS tile); knn 2, 10,
16 and knn > n; a lattice whose fourth neighbour is an exact tie across the tile edge and inside a tile; collinear and
coincident neighbourhoods; NaN and infinite points.  With knn = 2 (and n < 3) a neighbourhood is a segment or a point, no gap
exists and only the properties are held: unit length, and across the segment within 1e-6.

ICP: status and iterations equal, T within 1e-6 per entry, T = the guess on a failure (the bar of tests/test_gpu_icp3.py).
Shapes (1024 threads per job, a target tile of 4096 points in LDS, normals gathered from HBM): source counts 1, 64, 1023, 1024,
1025 on 300 targets; target counts 4095, 4096, 4097, 8193 under 200 sources; normals_knn 2, 10, 16; status 5 on a z = 0, a
one-wall and a collinear target and on 1 and 2 target points; statuses 1 and 2, a NaN in the guess; Counter and Differential
stops on either side of smoothLength; the slide along a wall; one launch of 8 jobs sharing targets with status-5 jobs among
them; 30 guesses on 700 x 900; the store route; the refusals."""
import numpy as np
import pytest

from sonar_slam_amd import _lib as L
from sonar_slam_amd import icp_config, pcl, store
from sonar_slam_amd.pipeline import ScanMatchBatch

import icp3_cases as C3
import icp3_plane_cases as C
import icp3_plane_ref as R

pytestmark = pytest.mark.gpu

TOL_TIGHT = 1e-6
TOL_NORMAL = 2.0 ** -23
ERR_ARG = r"libsonarfe error %d:" % L.SFE_ERR_ARG
f32 = np.float32


# ---- normals ----
def _hold_normals(got, want, gap, info, min_share=0.0):
    assert got.shape == want.shape and got.dtype == np.float32, info
    g = got.astype(np.float64)
    assert np.isfinite(g).all(), info
    assert np.abs(np.linalg.norm(g, axis=1) - 1.0).max(initial=0.0) < 1e-6, info
    cmp = gap >= C.GAP
    err = np.minimum(np.abs(g - want).max(axis=1), np.abs(g + want).max(axis=1))[cmp]
    print(info, "compared", int(cmp.sum()), "of", len(got), "worst", float(err.max(initial=0.0)))
    assert cmp.mean() >= min_share if len(got) else True, info
    assert err.max(initial=0.0) <= TOL_NORMAL, (info, float(err.max()))


def _across_the_nearest(cloud, got):
    """knn = 2: every normal is across the segment to the point's nearest neighbour"""
    ids = R.knn(tuple(cloud[:, a].copy() for a in range(3)), 2)
    d = cloud[ids[:, 1]].astype(np.float64) - cloud[ids[:, 0]].astype(np.float64)
    d /= np.linalg.norm(d, axis=1)[:, None]
    return np.abs((got.astype(np.float64) * d).sum(1)).max()


@pytest.mark.parametrize("knn", C.NORMALS_KNN)
@pytest.mark.parametrize("n", C.NORMALS_SIZES)
def test_surface_normals(ctx, n, knn):
    cloud = C.normals_cloud(n)
    got = pcl.surface_normals(cloud, knn, ctx=ctx)
    want, gap = C.normals_ref(n, knn)
    _hold_normals(got, want, gap, "normals n=%d knn=%d" % (n, knn), min_share=0.95 if min(n, knn) >= 3 else 0.0)
    if n == 1:
        assert np.array_equal(got, [[1, 0, 0]])
    elif min(n, knn) == 2:
        assert _across_the_nearest(cloud, got) < 1e-6


def test_surface_normals_knn_above_n(ctx):
    cloud = C.normals_cloud(5)
    got = pcl.surface_normals(cloud, 10, ctx=ctx)                     # the neighbourhood is the whole cloud
    want, gap = R.normals(cloud, 10, with_gap=True)
    _hold_normals(got, want, gap, "normals n=5 knn=10", min_share=1.0)
    assert np.array_equal(got, pcl.surface_normals(cloud, 5, ctx=ctx))


def test_surface_normals_ties_go_to_the_lowest_index(ctx):
    # (tests/test_icp3_plane_host.py: the other choice turns the centre normals by a right angle)
    cloud, knn, ties = C.lattice_tie_cloud()
    got = pcl.surface_normals(cloud, knn, ctx=ctx)
    want, gap = R.normals(cloud, knn, with_gap=True)
    _hold_normals(got, want, gap, "lattice")
    for c, chosen, refused in ties:
        assert gap[c] >= C.GAP and abs(float(got[c].astype(np.float64) @ want[c])) > 0.999


def test_surface_normals_of_degenerate_neighbourhoods(ctx):
    cloud, knn, same, run, d = C.degenerate_cloud()
    got = pcl.surface_normals(cloud, knn, ctx=ctx)
    want, gap = R.normals(cloud, knn, with_gap=True)
    _hold_normals(got, want, gap, "degenerate")                      # finite and unit everywhere; compared where a gap exists
    assert np.array_equal(got[same], np.tile([1, 0, 0], (len(same), 1)))               # C = 0
    assert np.abs(got[run].astype(np.float64) @ d).max() < 1e-6                         # across the line


def test_surface_normals_with_non_finite_points(ctx):
    cloud, knn, bad = C.nonfinite_cloud()
    got = pcl.surface_normals(cloud, knn, ctx=ctx)
    want, gap = R.normals(cloud, knn, with_gap=True)
    _hold_normals(got, want, gap, "nonfinite", min_share=0.9)
    assert np.array_equal(got[bad], np.tile([1, 0, 0], (len(bad), 1)))                 # nobody's neighbour, not their own


# ---- ICP ----
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


def test_three_wall_corner(ctx):
    s, t, g, p = C.job("knn10")
    msg, T = _icp(ctx, p).compute(s, t, g)
    assert msg == "success" and _diff(T, C.ref("knn10")[1]) < TOL_TIGHT and _diff(T, C3.TRUTH) < 2e-2


@pytest.mark.parametrize("ns", [1, 64, C.THREADS - 1, C.THREADS, C.THREADS + 1])
def test_source_counts(ctx, ns):
    _run(ctx, "ns%d" % ns)


@pytest.mark.parametrize("nt", [C.TILE - 1, C.TILE, C.TILE + 1, 2 * C.TILE + 1])
def test_target_counts(ctx, nt):
    _run(ctx, "nt%d" % nt)


@pytest.mark.parametrize("knn", [2, 10, 16])
def test_normals_knn(ctx, knn):
    st, T, it = _run(ctx, "knn%d" % knn)
    if knn == 2:      # the subset under the identity guess: b = 0, theta = 0
        assert st == 0 and _diff(T, np.eye(4)) < TOL_TIGHT


def test_source_that_is_a_subset_of_the_target_under_the_identity(ctx):
    st, T, it = _run(ctx, "subset")                                  # b = 0, theta = 0: no NaN from the rotation
    assert st == 0 and it == C.params().smooth_len and _diff(T, np.eye(4)) < TOL_TIGHT


@pytest.mark.parametrize("name", sorted(C.singular_jobs()))
def test_rank_deficient_targets_report_status_5(ctx, name):
    st, T, it = _run(ctx, name)
    assert (st, it) == (5, 0)
    s, t, g, p = C.job(name)
    msg, T1 = _icp(ctx, p).compute(s, t, g)
    assert msg == L.ICP_STATUS_MESSAGES[5] and np.array_equal(T1, g)


@pytest.mark.parametrize("name", sorted(C.status_jobs()))
def test_statuses_and_stops(ctx, name):
    st, T, it = _run(ctx, name)
    s, t, g, p = C.job(name)
    msg, T1 = _icp(ctx, p).compute(s, t, g)
    assert msg == L.ICP_STATUS_MESSAGES[st] and np.array_equal(T1, T, equal_nan=True)


def test_sliding_along_a_wall(ctx):
    # (tests/test_icp3_plane_host.py::test_sliding_along_a_wall asserts both facts from the references first)
    s, t, g, pp, p0 = C.sliding_job()
    st, T, it = _run(ctx, "sliding")
    m0, T0, it0 = _icp(ctx, p0).compute_batch(s, t, [g])
    print("sliding: point-to-plane", it, _diff(T, np.eye(4)), "point-to-point", int(it0[0]), _diff(T0[0], np.eye(4)))
    assert st == 0 and _diff(T, np.eye(4)) < 1e-3
    assert m0 == ["success"] and it < it0[0]


def test_one_launch_mixing_jobs(ctx):
    srcs, tgts, jobs, p = C.mixed_launch()
    icp = _icp(ctx, p)
    single = [icp.compute_batch(srcs[a], tgts[b], [g]) for a, b, g in jobs]
    for k, (a, b, g) in enumerate(jobs):
        msgs, T, it = single[k]
        want = C.ref("mixed%d" % k)
        assert msgs[0] == L.ICP_STATUS_MESSAGES[want[0]]
        _hold((want[0], T[0], it[0]), want, g, "mixed%d" % k)
    assert sorted(set(C.ref("mixed%d" % k)[0] for k in range(len(jobs)))) == [0, 5]
    msgs, T, it = icp.compute_pairs([srcs[a] for a, b, g in jobs], [tgts[b] for a, b, g in jobs], [g for a, b, g in jobs])
    for k in range(len(jobs)):
        assert msgs[k] == single[k][0][0] and np.array_equal(T[k], single[k][1][0]) and it[k] == single[k][2][0], k
    so = np.concatenate([[0], np.cumsum([len(s) for s in srcs])])
    to = np.concatenate([[0], np.cumsum([len(t) for t in tgts])])
    j4 = np.array([(so[a], len(srcs[a]), to[b], len(tgts[b])) for a, b, g in jobs], np.int32)
    st, T2, it2 = icp.compute_jobs(np.concatenate(srcs), np.concatenate(tgts), j4, np.stack([g for a, b, g in jobs]).reshape(-1, 16))
    for k in range(len(jobs)):
        assert st[k] == C.ref("mixed%d" % k)[0]
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
        msg, T1 = icp.compute(s, t, g)                               # the normals taken once for 30 jobs, or for this one
        assert msg == msgs[k] and np.array_equal(T1, T[k]), k
    assert len(set(int(i) for i in it)) > 1


def test_store_route_is_the_host_pointer_call(ctx):
    srcs, tgts, jobs, p = C.mixed_launch()
    clouds = srcs + tgts
    st3 = store.CloudStore3(ctx, capacity_points=sum(len(c) for c in clouds), max_clouds=len(clouds))
    try:
        h = [st3.put(c) for c in clouds]
        pairs = np.array([(h[a], h[len(srcs) + b]) for a, b, g in jobs], np.int32)
        gs = np.stack([g for a, b, g in jobs])
        for arg in (p, icp_config.IcpChain(p)):
            st, T, it = st3.icp(pairs, gs, arg)
            so = np.concatenate([[0], np.cumsum([len(s) for s in srcs])])
            to = np.concatenate([[0], np.cumsum([len(t) for t in tgts])])
            j4 = np.array([(so[a], len(srcs[a]), to[b], len(tgts[b])) for a, b, g in jobs], np.int32)
            st2, T2, it2 = _icp(ctx, p).compute_jobs(np.concatenate(srcs), np.concatenate(tgts), j4, gs.reshape(-1, 16))
            assert np.array_equal(st, st2) and np.array_equal(T, T2) and np.array_equal(it, it2)
            assert sorted(set(int(x) for x in st)) == [0, 5]
    finally:
        st3.close()


def test_refusals_reach_no_kernel(ctx):
    c3, c2 = np.zeros((5, 3), f32), np.zeros((5, 2), f32)
    j = np.array([[0, 5, 0, 5]], np.int32)
    # minimizer 1 on N x 3: the C entry point refuses it (SFE_ERR_ARG)
    icp = _icp(ctx, icp_config.shipped_params(minimizer=1))
    with pytest.raises(L.SonarFEError, match="point-to-point"):
        icp._call3(ctx, c3, c3, j, np.eye(4, dtype=f32).reshape(1, 16), np.zeros((1, 4, 4), f32), np.zeros(1, np.int32),
                   np.zeros(1, np.int32))
    # minimizer 2 with normals_knn outside [2, 16]
    for knn in (1, 17):
        with pytest.raises(L.SonarFEError, match=ERR_ARG):
            _icp(ctx, icp_config.shipped_params(minimizer=2, normals_knn=knn)).compute(c3, c3, np.eye(4, dtype=f32))
    # every 2-D entry point refuses minimizer 2
    p2 = icp_config.shipped_params(minimizer=2)
    g9 = np.eye(3, dtype=f32).reshape(1, 9)
    off = np.array([0, 5], np.int32)
    T, st, it = np.zeros((1, 3, 3), f32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    stage = L.IcpDpf(kind=L.DPF_MAX_DIST, dim=-1, remove_inside=0)
    stage.f[0] = 20.0
    chains = [icp_config.IcpChain(p2), icp_config.IcpChain(p2, reading=[stage]), icp_config.IcpChain(p2, reference=[stage]),
              icp_config.IcpChain(p2, outliers=L.IcpOutliers(use_median=1, median_factor=3.0))]
    for chain in chains:
        icp2 = pcl.ICP(ctx=ctx)
        icp2.setChain(chain)
        for shape, clouds in (("guesses", (L.ptr(c2, L.C.c_float), 5, L.ptr(c2, L.C.c_float), 5)),
                              ("pairs", (L.ptr(c2, L.C.c_float), L.ptr(off, L.C.c_int32), L.ptr(c2, L.C.c_float),
                                         L.ptr(off, L.C.c_int32))),
                              ("jobs", (L.ptr(c2, L.C.c_float), 5, L.ptr(c2, L.C.c_float), 5, L.ptr(j, L.C.c_int32)))):
            with pytest.raises(L.SonarFEError, match=ERR_ARG):
                icp2._call(ctx, shape, clouds, g9, 1, T, st, it)
    s2 = store.CloudStore(ctx, capacity_points=64, max_clouds=4)
    try:
        h = s2.put(np.zeros((5, 2), f32))
        for chain in (p2, chains[1], chains[3]):
            with pytest.raises(L.SonarFEError, match=ERR_ARG):
                s2.icp(chain, np.array([[h, h]], np.int32), g9.reshape(1, 3, 3))
    finally:
        s2.close()
    b = ScanMatchBatch(ctx, p2, [c2], [c2], [(0, 0)], [np.eye(3, dtype=f32)])          # sfe_icp_jobs_dev
    try:
        with pytest.raises(L.SonarFEError, match=ERR_ARG):
            b.run()
    finally:
        b.free()
