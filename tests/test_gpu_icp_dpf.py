"""GPU: the data-point filters of an ICP chain (sfe_icp_dpf.hip).

The filter pass (sfe_icp_filter_clouds_dev) against the numpy restatement of the predicate stages (tests/dpf_ref.py,
bit for bit, points one ulp either side of every threshold) and against pcl.downsample for the octree stage; ICP with
a chain against the plain ICP entry points run on clouds filtered beforehand (status, iterations and T bit for bit:
ICP with a chain IS ICP on the filtered clouds) and against the oracle in fp64-sum mode; the libpointmatcher form of
the point-to-plane chain against the implicit-normal chain; the routes the filtered sizes select; and the statuses of
jobs whose clouds the filters empty or whose octree is too deep."""
import ctypes as C

import numpy as np
import pytest

import oracle
from sonar_slam_amd import _lib as L
from sonar_slam_amd import icp_config, pcl, synth

from dpf_ref import apply, keep_mask, stage

pytestmark = pytest.mark.gpu

TOL_TIGHT = 1e-6
P2P_REC = dict(max_iter=30, use_diff_checker=0)   # the launcher's long-chain rules (tiny: <= 120000 point pairs)


def _nx(a, toward):
    return np.nextafter(np.float32(a), np.float32(toward), dtype=np.float32)


def filter_clouds(ctx, clouds, stages):
    """sfe_icp_filter_clouds_dev on clouds uploaded back to back -> (list of clouds | None where refused, counts)"""
    clouds = [np.ascontiguousarray(c, np.float32).reshape(-1, 2) for c in clouds]
    off = np.zeros(len(clouds) + 1, np.int32)
    off[1:] = np.cumsum([len(c) for c in clouds])
    pts = np.concatenate(clouds) if off[-1] else np.zeros((1, 2), np.float32)
    d_in = ctx.alloc(max(pts.nbytes, 8))
    d_in.upload(pts)
    d_out = ctx.alloc(max(pts.nbytes, 8))
    arr, n = icp_config.IcpChain.device_stages(stages)
    counts = np.zeros(len(clouds), np.int32)
    with ctx.lock:
        ctx._check(ctx.lib.sfe_icp_filter_clouds_dev(ctx.handle, arr, n, d_in.ptr, L.ptr(off, C.c_int32), len(clouds),
                                                     d_out.ptr, L.ptr(counts, C.c_int32)))
        total = int(np.maximum(counts, 0).sum())
        flat = d_out.download(np.float32, 2 * total).reshape(-1, 2) if total else np.zeros((0, 2), np.float32)
    out, at = [], 0
    for k in counts:
        out.append(None if k < 0 else flat[at:at + k])
        at += max(int(k), 0)
    d_in.free()
    d_out.free()
    return out, counts


def _ds(ctx):
    return lambda p, res: pcl.downsample(p, res, ctx=ctx)


def _threshold_cloud(rng, n):
    """points on and one ulp either side of the thresholds of PRED_STAGES"""
    base = []
    for v in (5.0, -2.0, 2.0, 1.5, -1.5, 3.0):
        for w in (v, _nx(v, 100), _nx(v, -100)):
            base += [[w, 0.5], [0.5, w], [-w, 0.25], [0.25, -w]]
    for r in (12.0, 4.0):        # on the circles of the norm stages: (0.6 r, 0.8 r) and neighbours
        for sx in (0.6, _nx(0.6, 1), _nx(0.6, 0)):
            base.append([np.float32(sx) * np.float32(r), np.float32(0.8) * np.float32(r)])
        base += [[r, 0], [_nx(r, 0), 0], [_nx(r, 100), 0], [0, -r], [0, _nx(-r, 0)]]
    base = np.asarray(base, np.float32)
    return np.concatenate([base, rng.uniform(-15, 15, (max(n - len(base), 0), 2)).astype(np.float32)])[:max(n, len(base))]


PRED_CHAINS = {
    "maxdist_norm": [stage(L.DPF_MAX_DIST, -1, f=[12.0])],
    "mindist_norm": [stage(L.DPF_MIN_DIST, -1, f=[-4.0])],
    "maxdist_x_y": [stage(L.DPF_MAX_DIST, 0, f=[5.0]), stage(L.DPF_MAX_DIST, 1, f=[-2.0])],
    "mindist_x_y": [stage(L.DPF_MIN_DIST, 0, f=[-1.5]), stage(L.DPF_MIN_DIST, 1, f=[2.0])],
    "box_remove": [stage(L.DPF_BOUNDING_BOX, remove_inside=1, f=[-2.0, 3.0, -1.5, 5.0, -1, 1])],
    "box_keep": [stage(L.DPF_BOUNDING_BOX, remove_inside=0, f=[-2.0, 3.0, -1.5, 5.0, -1, 1])],
    "all": [stage(L.DPF_MIN_DIST, -1, f=[4.0]), stage(L.DPF_MAX_DIST, -1, f=[12.0]),
            stage(L.DPF_BOUNDING_BOX, remove_inside=1, f=[-2.0, 3.0, -1.5, 5.0, -1, 1]),
            stage(L.DPF_MAX_DIST, 0, f=[5.0])],
}


@pytest.mark.parametrize("name", sorted(PRED_CHAINS))
def test_predicate_stages_bit_for_bit(ctx, name):
    rng = np.random.default_rng(7)
    st = PRED_CHAINS[name]
    clouds = [_threshold_cloud(rng, n) for n in (1, 64, 65, 1000, 5000, 20000)]
    clouds += [rng.uniform(-20, 20, (n, 2)).astype(np.float32) for n in (1, 2, 255, 256, 1023, 1025, 4097)]
    clouds += [synth.scan_pair(seed=s, n_src=3000, n_tgt=2000)[k] for s in (1, 2) for k in (0, 1)]
    clouds.append(np.zeros((0, 2), np.float32))
    out, counts = filter_clouds(ctx, clouds, st)
    for c, o in zip(clouds, out):
        want = apply(c, st)
        assert o is not None and o.shape == want.shape and np.array_equal(o.view(np.uint32), want.view(np.uint32))
    # the threshold points really sit on both sides
    m = keep_mask(clouds[0], st[0])
    assert m.any() and not m.all()


@pytest.mark.parametrize("res", [0.5, 0.1])
def test_octree_stage_equals_downsample(ctx, res):
    rng = np.random.default_rng(11)
    clouds = [rng.uniform(-30, 30, (n, 2)).astype(np.float32) for n in (1, 3, 700, 5000)]
    clouds += [synth.scan_pair(seed=3, n_src=20000, n_tgt=9000)[k] for k in (0, 1)]   # 20 000: the HBM-scratch sort
    out, counts = filter_clouds(ctx, clouds, [stage(L.DPF_OCTREE_GRID, f=[res])])
    for c, o in zip(clouds, out):
        want = pcl.downsample(c, res, ctx=ctx)
        assert o is not None and np.array_equal(o, want)


def test_mixed_chain_is_the_composition(ctx):
    rng = np.random.default_rng(12)
    st = [stage(L.DPF_MAX_DIST, -1, f=[25.0]), stage(L.DPF_OCTREE_GRID, f=[0.3]),
          stage(L.DPF_BOUNDING_BOX, remove_inside=1, f=[-1, 1, -1, 1, 0, 0]), stage(L.DPF_OCTREE_GRID, f=[0.7]),
          stage(L.DPF_MIN_DIST, 0, f=[0.5])]
    clouds = [synth.scan_pair(seed=s, n_src=n, n_tgt=10)[0] for s, n in ((4, 1), (5, 900), (6, 5000), (7, 20000))]
    clouds.append(rng.uniform(-40, 40, (3000, 2)).astype(np.float32))
    out, _ = filter_clouds(ctx, clouds, st)
    for c, o in zip(clouds, out):
        assert np.array_equal(o, apply(c, st, _ds(ctx)))


def test_octree_deeper_than_24_levels_reports_minus_one(ctx):
    rng = np.random.default_rng(13)
    wide = rng.uniform(-30, 30, (600, 2)).astype(np.float32)
    small = rng.uniform(0, 0.01, (300, 2)).astype(np.float32)
    out, counts = filter_clouds(ctx, [small, wide, small], [stage(L.DPF_OCTREE_GRID, f=[1e-6]),
                                                            stage(L.DPF_MAX_DIST, f=[100.0])])
    assert counts[1] == -1 and out[1] is None
    assert counts[0] > 0 and np.array_equal(out[0], pcl.downsample(small, 1e-6, ctx=ctx)) and np.array_equal(out[0], out[2])


# ---- ICP with a chain == ICP on the clouds filtered beforehand -----------------------------------------------------
SIDE_STAGES = {
    "maxdist": [stage(L.DPF_MAX_DIST, -1, f=[18.0])],
    "mindist": [stage(L.DPF_MIN_DIST, 1, f=[0.5])],
    "box": [stage(L.DPF_BOUNDING_BOX, remove_inside=1, f=[-3.0, 3.0, -3.0, 3.0, -1, 1])],
    "octree": [stage(L.DPF_OCTREE_GRID, f=[0.4])],
}


def _icp(ctx, params, reading=(), reference=()):
    icp = pcl.ICP(ctx)
    icp.setChain(icp_config.IcpChain(params, reading, reference))
    return icp


def _plain(ctx, params):
    icp = pcl.ICP(ctx)
    icp.setParams(params)
    return icp


def _same(a, b):
    (ma, Ta, ia), (mb, Tb, ib) = a, b
    assert list(ma) == list(mb)
    assert np.array_equal(np.asarray(ia), np.asarray(ib))
    assert np.array_equal(np.asarray(Ta).view(np.uint32), np.asarray(Tb).view(np.uint32))


@pytest.mark.parametrize("minimizer", [0, 1])
@pytest.mark.parametrize("side", ["reading", "reference"])
@pytest.mark.parametrize("kind", sorted(SIDE_STAGES))
def test_compute_with_a_filter_on_one_side(ctx, kind, side, minimizer):
    src, tgt, guess, _ = synth.scan_pair(seed=20, n_src=2500, n_tgt=2400)
    p = icp_config.shipped_params(minimizer=minimizer)
    st = SIDE_STAGES[kind]
    rd, rf = (st, []) if side == "reading" else ([], st)
    chain = _icp(ctx, p, rd, rf)
    fs, ft = apply(src, rd, _ds(ctx)), apply(tgt, rf, _ds(ctx))
    assert len(fs) < len(src) or len(ft) < len(tgt)
    msg, T = chain.compute(src, tgt, guess)
    msg0, T0 = _plain(ctx, p).compute(fs, ft, guess)
    assert msg == msg0 and np.array_equal(T.view(np.uint32), T0.view(np.uint32))
    _same(chain.compute_batch(src, tgt, [guess]), _plain(ctx, p).compute_batch(fs, ft, [guess]))


@pytest.mark.parametrize("minimizer", [0, 1])
def test_compute_batch_30_guesses_and_the_oracle(ctx, minimizer):
    src, tgt, guess, _ = synth.scan_pair(seed=21, n_src=3000, n_tgt=3000)
    rng = np.random.default_rng(21)
    gs = [(guess.astype(np.float64) @ synth.pose_matrix(*rng.normal(0, [0.2, 0.2, 0.02]))).astype(np.float32)
          for _ in range(30)]
    p = icp_config.shipped_params(minimizer=minimizer)
    rd = [stage(L.DPF_MAX_DIST, -1, f=[20.0]), stage(L.DPF_OCTREE_GRID, f=[0.25])]
    rf = [stage(L.DPF_OCTREE_GRID, f=[0.2]), stage(L.DPF_BOUNDING_BOX, remove_inside=1, f=[-2, 2, -2, 2, 0, 0])]
    got = _icp(ctx, p, rd, rf).compute_batch(src, tgt, gs)
    fs, ft = apply(src, rd, _ds(ctx)), apply(tgt, rf, _ds(ctx))
    _same(got, _plain(ctx, p).compute_batch(fs, ft, gs))
    msgs, T, it = got
    for k in range(0, 30, 7):
        st_o, To, ito = oracle.icp(fs, ft, gs[k], oracle.shipped_icp_params(minimizer=minimizer, precision=1))
        assert L.ICP_STATUS_MESSAGES[st_o] == msgs[k] and ito == it[k]
        a, b = synth.pose_of(T[k]), synth.pose_of(To)
        assert max(abs(x - y) for x, y in zip(a, b)) < TOL_TIGHT


def test_compute_pairs_and_jobs_with_shared_slices(ctx):
    pairs = [synth.scan_pair(seed=30 + s, n_src=n, n_tgt=m) for s, (n, m) in enumerate([(800, 900), (3000, 2500),
                                                                                         (5000, 5000), (300, 350)])]
    p = icp_config.shipped_params()
    rd = [stage(L.DPF_MIN_DIST, -1, f=[1.0])]
    rf = [stage(L.DPF_MAX_DIST, -1, f=[22.0]), stage(L.DPF_OCTREE_GRID, f=[0.3])]
    chain = _icp(ctx, p, rd, rf)
    srcs, tgts, gs = [q[0] for q in pairs], [q[1] for q in pairs], [q[2] for q in pairs]
    fsrcs = [apply(s, rd, _ds(ctx)) for s in srcs]
    ftgts = [apply(t, rf, _ds(ctx)) for t in tgts]
    _same(chain.compute_pairs(srcs, tgts, gs), _plain(ctx, p).compute_pairs(fsrcs, ftgts, gs))
    # a job table over shared pools: every source against two targets, target 2 named by five jobs
    so = np.r_[0, np.cumsum([len(s) for s in srcs])]
    to = np.r_[0, np.cumsum([len(t) for t in tgts])]
    fso = np.r_[0, np.cumsum([len(s) for s in fsrcs])]
    fto = np.r_[0, np.cumsum([len(t) for t in ftgts])]
    table = [(i, j) for i in range(4) for j in (i, 2)] + [(2, 2), (0, 3)]
    jobs = np.array([(so[i], len(srcs[i]), to[j], len(tgts[j])) for i, j in table], np.int32)
    fjobs = np.array([(fso[i], len(fsrcs[i]), fto[j], len(ftgts[j])) for i, j in table], np.int32)
    g9 = np.stack([gs[i].reshape(9) for i, _ in table]).astype(np.float32)
    st, T, it = chain.compute_jobs(np.concatenate(srcs), np.concatenate(tgts), jobs, g9)
    st0, T0, it0 = _plain(ctx, p).compute_jobs(np.concatenate(fsrcs), np.concatenate(ftgts), fjobs, g9)
    assert np.array_equal(st, st0) and np.array_equal(it, it0) and np.array_equal(T.view(np.uint32), T0.view(np.uint32))
    assert (st == 0).sum() >= len(table) // 2


@pytest.mark.parametrize("knn", [10, 6])
def test_libpointmatcher_form_point_to_plane(ctx, tmp_path, knn):
    from test_icp_chain_host import lpm_point_to_plane
    f = tmp_path / "icp.yaml"
    f.write_text(lpm_point_to_plane(knn))
    icp = pcl.ICP(ctx)
    icp.loadFromYaml(str(f))
    assert icp.params.minimizer == 1 and icp.params.normals_knn == knn
    src, tgt, guess, _ = synth.scan_pair(seed=40, n_src=2000, n_tgt=2000)
    p = icp_config.shipped_params(minimizer=1, normals_knn=knn)
    _same(icp.compute_batch(src, tgt, [guess, guess @ synth.pose_matrix(0.1, 0, 0.01).astype(np.float32)]),
          _plain(ctx, p).compute_batch(src, tgt, [guess, guess @ synth.pose_matrix(0.1, 0, 0.01).astype(np.float32)]))


def _radius_keeping(cloud, k):
    """a MaxDist (dim -1) threshold that keeps exactly the k points nearest the origin (distinct norms assumed)"""
    nrm = np.sqrt(np.float32(cloud[:, 0] * cloud[:, 0]) + np.float32(cloud[:, 1] * cloud[:, 1]), dtype=np.float32)
    return float(np.sort(nrm)[k])


@pytest.mark.parametrize("route,k_src,k_tgt", [(L.ICP_ROUTE_T0, 380, 500), (L.ICP_ROUTE_T1, 1500, 1600),
                                               (L.ICP_ROUTE_TINY, 200, 250)])
def test_routes_follow_the_filtered_sizes(ctx, route, k_src, k_tgt):
    src, tgt, guess, _ = synth.scan_pair(seed=50, n_src=5000, n_tgt=5000)
    n = 2 * ctx.n_cu + 8
    rng = np.random.default_rng(50)
    gs = [(guess.astype(np.float64) @ synth.pose_matrix(*rng.normal(0, [0.05, 0.05, 0.005]))).astype(np.float32)
          for _ in range(n)]
    p = icp_config.shipped_params(**P2P_REC)
    rd = [stage(L.DPF_MAX_DIST, -1, f=[_radius_keeping(src, k_src)])]
    rf = [stage(L.DPF_MAX_DIST, -1, f=[_radius_keeping(tgt, k_tgt)])]
    fs, ft = apply(src, rd), apply(tgt, rf)
    assert (len(fs), len(ft)) == (k_src, k_tgt)
    got = _icp(ctx, p, rd, rf).compute_batch(src, tgt, gs)
    routes = ctx.icp_routes(n)
    assert (routes == route).all(), np.unique(routes)
    want = _plain(ctx, p).compute_batch(fs, ft, gs)
    assert (ctx.icp_routes(n) == route).all()
    _same(got, want)


def test_empty_and_too_deep_jobs_report_their_status(ctx):
    rng = np.random.default_rng(60)
    src0, tgt0, g0, _ = synth.scan_pair(seed=60, n_src=600, n_tgt=600)
    s = np.float32(1e-3)                               # the targets: a 0.03 m patch (octree fine at 1e-6) ...
    tgt_small = (tgt0 * s).astype(np.float32)
    src_small = (src0 * s).astype(np.float32)
    far = rng.uniform(200, 300, (400, 2)).astype(np.float32)        # ... a reading the MaxDist stage empties
    tgt_wide = rng.uniform(-30, 30, (500, 2)).astype(np.float32)   # ... a reference 26 levels deep
    g0s = g0.copy()
    g0s[:2, 2] *= s
    g = [g0s, np.eye(3, dtype=np.float32), g0s, (g0s @ synth.pose_matrix(1, 2, 0.3)).astype(np.float32)]
    p = icp_config.shipped_params(matcher_max_dist=1.0, max_dist_filter=0.01)
    rd = [stage(L.DPF_MAX_DIST, 0, f=[100.0])]
    rf = [stage(L.DPF_OCTREE_GRID, f=[1e-6])]
    msgs, T, it = _icp(ctx, p, rd, rf).compute_pairs([src_small, far, src_small, far], [tgt_small, tgt_small,
                                                                                         tgt_wide, tgt_wide], g)
    assert msgs[1] == L.ICP_STATUS_MESSAGES[7] and msgs[2] == L.ICP_STATUS_MESSAGES[8]
    assert msgs[3] in (L.ICP_STATUS_MESSAGES[7], L.ICP_STATUS_MESSAGES[8])
    for k in (1, 2, 3):
        assert np.array_equal(T[k], g[k]) and it[k] == 0
    routes = ctx.icp_routes(4)
    assert (routes[1:] == -1).all() and routes[0] >= 0
    # the job that ran is the one the plain path runs on its filtered clouds
    want = _plain(ctx, p).compute_pairs([apply(src_small, rd)], [pcl.downsample(tgt_small, 1e-6, ctx=ctx)], [g[0]])
    _same((msgs[:1], T[:1], it[:1]), want)
