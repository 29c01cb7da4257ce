"""GPU: ``pcl.ICP`` on N x 3 clouds with 4 x 4 guesses (sfe_icp3.hip) against the numpy restatement of its rules
(tests/icp3_ref.py): status and iterations equal, T within 1e-6 per entry (the bar of tests/test_gpu_icp_outliers.py), T = the
guess on a failure.  The inputs are built in tests/icp3_cases.py; tests/test_icp3_ref_host.py holds every one of them to the
input-stability check (the reference with its sums reversed lands on itself), so that the comparison stays off match and
quantile decision boundaries.

Shapes (the kernel: 1024 threads per job, one query per lane and pass, a target tile of 4096 points in LDS):
  source counts 1, 63, 64, 65, 1023, 1024, 1025 on 300 targets; target counts 4095, 4096, 4097, 8193 under 200 sources;
  exact ties across the tile edge (targets 4095 | 4096), inside a tile and between the second and third tile; NaN, infinite and
  out-of-range sources; trimmed ranks on a run of 100 equal distances and ratio 1; statuses 1 and 2, a NaN in the guess,
  Counter and Differential stops on either side of smoothLength, 80 iterations (history of 64); one launch of 8 jobs from 1 x
  8192 to 1500 x 4099 that share clouds, a failing one among them; 30 guesses on 700 x 900; z = 0 against the 2-D kernels;
  nearly planar clouds (the reference's reflection fix fires); 3000 x 5000 about a skew axis with outliers."""
import numpy as np
import pytest

from sonar_slam_amd import _lib as L
from sonar_slam_amd import icp_config, pcl

import icp3_cases as C
import icp3_ref

pytestmark = pytest.mark.gpu

TOL_TIGHT = 1e-6
f32 = np.float32


def _icp(ctx, p):
    icp = pcl.ICP(ctx=ctx)
    icp.setParams(p)
    return icp


def _diff(Ta, Tb):
    return float(np.abs(np.asarray(Ta, np.float64) - np.asarray(Tb, np.float64)).max())


def _hold(got, want, guess, info):
    """(status, T, iterations) of the device against the reference's"""
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
    """the named job through a one-job compute_jobs call (status as a number), held against the reference"""
    s, t, g, p = C.job(name)
    st, T, it = _icp(ctx, p).compute_jobs(s, t, np.array([[0, len(s), 0, len(t)]], np.int32), g.reshape(1, 16))
    _hold((st[0], T[0], it[0]), C.ref(name), g, name)
    return int(st[0]), T[0], int(it[0])


@pytest.mark.parametrize("ns", [1, 63, 64, 65, C.THREADS - 1, C.THREADS, C.THREADS + 1])
def test_source_counts(ctx, ns):
    _run(ctx, "ns%d" % ns)


@pytest.mark.parametrize("nt", [C.TILE - 1, C.TILE, C.TILE + 1, 2 * C.TILE + 1])
def test_target_counts(ctx, nt):
    _run(ctx, "nt%d" % nt)


def test_ties_go_to_the_lowest_index_across_and_inside_tiles(ctx):
    # (tests/test_icp3_ref_host.py::test_tie_case_depends_on_the_lowest_index: any other choice for one of the three tied
    # queries moves the pose by more than 100 x the bar)
    _run(ctx, "ties")


def test_non_finite_and_out_of_range_sources(ctx):
    _run(ctx, "nonfinite")


@pytest.mark.parametrize("ratio", ["0.5", "0.8", "1"])
def test_trimmed_rank_on_a_run_of_equal_distances(ctx, ratio):
    _run(ctx, "run" + ratio)


@pytest.mark.parametrize("name", sorted(C.status_jobs()))
def test_statuses_and_stops(ctx, name):
    st, T, it = _run(ctx, name)
    s, t, g, p = C.job(name)
    msg, T1 = _icp(ctx, p).compute(s, t, g)                      # ... and the message of the reference's binding
    assert msg == {0: "success", 1: "no outlier to filter", 2: "ErrorMnimizer: no point to minimize"}[st]
    assert np.array_equal(T1, T, equal_nan=True)


def test_one_launch_mixing_jobs(ctx):
    srcs, tgts, jobs, p = C.mixed_launch()
    icp = _icp(ctx, p)
    single = [icp.compute_batch(srcs[a], tgts[b], [g]) for a, b, g in jobs]
    for k, (a, b, g) in enumerate(jobs):
        msgs, T, it = single[k]
        want = C.ref("mixed%d" % k)
        assert msgs[0] == L.ICP_STATUS_MESSAGES[want[0]]
        _hold((want[0], T[0], it[0]), want, g, "mixed%d" % k)
    # compute_pairs: the same jobs in one launch (the clouds handed in again and again go up once)
    msgs, T, it = icp.compute_pairs([srcs[a] for a, b, g in jobs], [tgts[b] for a, b, g in jobs], [g for a, b, g in jobs])
    for k in range(len(jobs)):
        assert msgs[k] == single[k][0][0] and np.array_equal(T[k], single[k][1][0]) and it[k] == single[k][2][0], k
    # compute_jobs over pools, results into arrays handed in
    so = np.concatenate([[0], np.cumsum([len(s) for s in srcs])])
    to = np.concatenate([[0], np.cumsum([len(t) for t in tgts])])
    j4 = np.array([(so[a], len(srcs[a]), to[b], len(tgts[b])) for a, b, g in jobs], np.int32)
    out = (np.full(len(jobs), -7, np.int32), np.full((len(jobs), 4, 4), 9.0, f32), np.full(len(jobs), -7, np.int32))
    ret = icp.compute_jobs(np.concatenate(srcs), np.concatenate(tgts), j4, np.stack([g for a, b, g in jobs]).reshape(-1, 16),
                           out=out)
    assert all(r is o for r, o in zip(ret, out))
    for k in range(len(jobs)):
        assert out[0][k] == C.ref("mixed%d" % k)[0]
        assert np.array_equal(out[1][k], single[k][1][0]) and out[2][k] == single[k][2][0], k
    # a job slice outside the clouds is a bad argument, not a launch
    with pytest.raises(L.SonarFEError):
        icp.compute_jobs(np.concatenate(srcs), np.concatenate(tgts), np.array([[0, 5, 0, 10 ** 6]], np.int32),
                         np.eye(4, dtype=f32).reshape(1, 16))


def test_compute_batch_of_30_guesses(ctx):
    s, t, _ = C.pair(500, 700, 900)
    gs = C.batch_guesses()
    icp = _icp(ctx, C.params())
    msgs, T, it = icp.compute_batch(s, t, gs)
    assert T.shape == (30, 4, 4)
    for k, g in enumerate(gs):
        assert msgs[k] == L.ICP_STATUS_MESSAGES[C.ref("batch%d" % k)[0]]
        _hold((C.ref("batch%d" % k)[0], T[k], it[k]), C.ref("batch%d" % k), g, "batch%d" % k)
    for k in (0, 7, 29):
        msg, T1 = icp.compute(s, t, gs[k])
        assert msg == msgs[k] and np.array_equal(T1, T[k])
    assert len(set(int(i) for i in it)) > 1                      # not every guess takes the same number of steps


@pytest.mark.parametrize("k", range(3))
def test_planar_clouds_give_the_2d_result(ctx, k):
    _run(ctx, "planar%d" % k)
    s, t, g, p = C.job("planar%d" % k)
    icp = _icp(ctx, p)
    m3, T3, it3 = icp.compute_batch(s, t, [g])
    m2, T2, it2 = icp.compute_batch(s[:, :2].copy(), t[:, :2].copy(), [C.guess3(g)])
    assert m3 == m2 == ["success"] and it3[0] == it2[0]
    print("planar", k, "3-D against 2-D", _diff(T3[0], icp3_ref.embed(T2[0])))
    assert _diff(T3[0], icp3_ref.embed(T2[0])) < TOL_TIGHT


@pytest.mark.parametrize("k", range(4))
def test_nearly_planar_clouds(ctx, k):
    st, T, it = _run(ctx, "thin%d" % k)
    assert abs(np.linalg.det(T[:3, :3].astype(np.float64)) - 1.0) < 1e-5      # a proper rotation where U V^T is a reflection


def test_skew_axis_partial_overlap_outliers(ctx):
    st, T, it = _run(ctx, "skew")
    assert st == 0 and it > C.params().smooth_len


def test_refusals_reach_no_kernel(ctx):
    icp = _icp(ctx, icp_config.shipped_params(minimizer=1))
    c3 = np.zeros((5, 3), f32)
    with pytest.raises(NotImplementedError, match="PointToPlane"):
        icp.compute(c3, c3, np.eye(4, dtype=f32))
    # the C entry point refuses it too (SFE_ERR_ARG): the library never runs a point-to-plane chain on 3-D clouds
    with pytest.raises(L.SonarFEError, match="point-to-point"):
        icp._call3(ctx, c3, c3, np.array([[0, 5, 0, 5]], np.int32), np.eye(4, dtype=f32).reshape(1, 16),
                   np.zeros((1, 4, 4), f32), np.zeros(1, np.int32), np.zeros(1, np.int32))
