"""GPU: whole ICP chains (data-point filters, MinDist / MedianDist outlier filters, the Bound checker) on the resident
routes -- ``store.CloudStore.icp`` (sfe_icp_store_compute_chain_ext), ``replay.FrontEnd`` over a store,
``chained.SessionBatch`` and ``farm.IcpFarm`` -- bit for bit (status, iterations, T) what ``pcl.ICP`` with the same chain
computes on the same clouds.  Every chain is checked to change the results of the shipped chain on the data used, so a
chain a route drops silently cannot pass."""
import numpy as np
import pytest

from sonar_slam_amd import _lib as L
from sonar_slam_amd import icp_config, pcl, synth
from sonar_slam_amd import store as st

import resident_chains as R

pytestmark = pytest.mark.gpu

CHAINS = ("filters", "outliers", "plane", "empty")


def _pairs():
    """six scan pairs, and two clouds that lie at x < 0 (the 'empty' chain leaves nothing of them)"""
    ps = [synth.scan_pair(seed=40 + i, n_src=500 + 150 * i, n_tgt=700 + 100 * i) for i in range(6)]
    mirrored = [np.c_[-np.abs(c[:, 0]) - 2.0, c[:, 1]].astype(np.float32) for c in (ps[0][0], ps[1][1])]
    srcs = [p[0] for p in ps] + mirrored[:1]
    tgts = [p[1] for p in ps] + mirrored[1:]
    return srcs, tgts, [p[2] for p in ps]


def _noisy(g, rng, scale):
    return (np.asarray(g, np.float64) @ synth.pose_matrix(*rng.normal(0, [0.2 * scale, 0.2 * scale, 0.04 * scale]))
            ).astype(np.float32)


def _jobs(shape, name=None):
    """-> (source clouds, target clouds, pairs [n x 2] of cloud indices, guesses [n x 3 x 3])"""
    srcs, tgts, gs = _pairs()
    rng = np.random.default_rng(5)
    if shape == "shared":
        # many pairs over few handles: every cloud is named by several jobs, as source or target; poor guesses included
        pairs, guesses = [], []
        for j in range(40):
            a = j % len(srcs)
            b = a if (j % 3 or a >= len(gs)) else (a + 1) % len(gs)
            pairs.append((a, b))
            guesses.append(_noisy(gs[a % len(gs)], rng, 0.5 + 2.0 * (j % 4 == 3)))
    else:
        # the shape of FrontEnd.compute_icp_with_cov: 30 guesses on one pair
        pairs = [(6, 6) if name == "empty" else (2, 2)] * 30
        guesses = [_noisy(gs[2], rng, 1.0 + (j % 5 == 4)) for j in range(30)]
    return srcs, tgts, pairs, np.stack(guesses)


def _store(ctx, srcs, tgts):
    s = st.CloudStore(ctx, capacity_points=1 << 16, max_clouds=64)
    s.put(np.ones((3, 2), np.float32))                      # (not at the start of the pool)
    hs = [s.put(c) for c in srcs]
    ht = [s.put(c) for c in tgts]
    return s, np.array(hs), np.array(ht)


def _host(ctx, chain, s, hpairs, guesses):
    icp = pcl.ICP(ctx)
    icp.setChain(chain)
    msgs, T, it = icp.compute_pairs([s.read(a) for a, _ in hpairs], [s.read(b) for _, b in hpairs], list(guesses))
    status = np.array([{v: k for k, v in L.ICP_STATUS_MESSAGES.items()}[m] for m in msgs], np.int32)
    return T, status, it


def _equal(a, b, what):
    for k, name in enumerate(("T", "status", "iters")):
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, name, np.flatnonzero(
            (np.asarray(a[k]) != np.asarray(b[k])).reshape(len(a[1]), -1).any(axis=1))[:10])


def _differs(a, b):
    return any(not np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("shape", ["shared", "guesses"])
@pytest.mark.parametrize("name", CHAINS)
def test_store_chain_equals_pcl_icp_with_the_chain(ctx, name, shape):
    chain = R.chain(name)
    srcs, tgts, pairs, guesses = _jobs(shape, name)
    s, hs, ht = _store(ctx, srcs, tgts)
    hpairs = np.array([(hs[a], ht[b]) for a, b in pairs], np.int32)
    got = s.icp(chain, hpairs, guesses)
    want = _host(ctx, chain, s, hpairs, guesses)
    _equal(got, want, (name, shape))
    shipped = s.icp(icp_config.shipped_params(), hpairs, guesses)
    assert _differs(got, shipped), "the chain changes nothing on this data: a dropped chain would pass"
    status = got[1]
    if shape == "shared":
        assert (status == 0).sum() >= 10, status
        if name == "outliers":
            assert (status == L.ICP_BOUND).any(), status
        if name == "empty":
            assert (status == 7).any(), status
            bad = np.array([a >= 6 for a, _ in pairs])
            assert (status[bad] == 7).all() and (status[~bad] != 7).all()
            assert np.array_equal(got[0][bad], guesses[bad]) and (got[2][bad] == 0).all()
    s.close()


def test_module_free_chain_is_its_params_on_the_store(ctx):
    srcs, tgts, pairs, guesses = _jobs("shared")
    s, hs, ht = _store(ctx, srcs, tgts)
    hpairs = np.array([(hs[a], ht[b]) for a, b in pairs], np.int32)
    chain = R.chain("shipped")
    assert not chain.has_modules()
    _equal(s.icp(chain, hpairs, guesses), s.icp(chain.params, hpairs, guesses), "shipped")
    # point-to-plane with only the normals stage: nothing beyond IcpParams either
    plane = icp_config.parse_icp_chain(R.CHAINS["plane"].replace(
        "  - BoundingBoxDataPointsFilter: {xMin: -26.0, xMax: 26.0, yMin: -26.0, yMax: 26.0, zMin: -1.0, zMax: 1.0, "
        "removeInside: 0}\n", ""))
    assert not plane.has_modules() and plane.params.normals_knn == 8
    _equal(s.icp(plane, hpairs, guesses), s.icp(plane.params, hpairs, guesses), "plane")
    s.close()


def _records_equal(a, b):
    if isinstance(a, dict) and isinstance(b, dict):
        return set(a) == set(b) and all(_records_equal(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list, np.ndarray)) or isinstance(b, (tuple, list, np.ndarray)):
        if isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)) and len(a) == len(b) and any(
                isinstance(x, (dict, tuple, list)) for x in a):
            return all(_records_equal(x, y) for x, y in zip(a, b))
        a, b = np.asarray(a), np.asarray(b)
        return a.shape == b.shape and np.array_equal(a, b)
    return a == b


def _factors(front):
    return [f[:3] + ((f[3].x(), f[3].y(), f[3].theta()),) if len(f) > 3 else f[:2] for f in front.backend.factors]


def test_front_end_with_a_loaded_chain_on_the_store_equals_the_host_flow(ctx, tmp_path):
    """replay.FrontEnd(nssm_enable=True) with the chain installed by fe.icp.loadFromYaml AFTER construction: on a store
    (compute_icp and compute_icp_with_cov through store.icp) == without one (pcl.ICP), every record and every factor;
    and the log differs from the same replay under the shipped chain."""
    from sonar_slam_amd.feature_extraction import FeatureExtraction, SonarPing, oculus_bearings
    from sonar_slam_amd.replay import FrontEnd, replay
    path = tmp_path / "icp.yaml"
    path.write_text(R.CHAINS["replay"])
    K, rows, beams = 15, 256, 128
    bearings = oculus_bearings(beams)
    world = synth.world_structure(seed=2, n=9000)
    true, dr = synth.trajectory(n=K, step=1.7, turn=2 * np.pi / 13, seed=21, start=(20.0, 0.0, 0.0))
    pings = [SonarPing(synth.render_ping(world, true[k], bearings, rows=rows, seed=k), bearings, 30.0 / rows, ping_id=k)
             for k in range(K)]

    def run(use_store, load):
        fe = FeatureExtraction(ctx)
        fe.Ntc, fe.Ngc, fe.Pfa, fe.rank, fe.alg, fe.threshold = 40, 10, 0.1, 10, "SOCA", 65
        fe.resolution, fe.outlier_filter_radius, fe.outlier_filter_min_points, fe.skip = 0.5, 1.0, 5, 1
        fe.configure()
        s = st.CloudStore(ctx, capacity_points=1 << 18, max_clouds=256) if use_store else None
        front = FrontEnd(ctx, keyframe_translation=1.5, keyframe_duration=0.5, store=s, ssm_min_points=20, nssm_enable=True,
                         nssm_min_points=30, mcd_random_state=0)
        if load:
            front.icp.loadFromYaml(str(path))
        log, _, _ = replay(pings, np.arange(K, dtype=float), dr, fe, front)
        if s is not None:
            s.close()
        return log, _factors(front)

    host, dev, shipped = run(False, True), run(True, True), run(True, False)
    assert len(host[0]) == len(dev[0]) == K
    for ra, rb in zip(host[0], dev[0]):
        if rb.get("nssm"):
            rb = dict(rb, nssm={k: v for k, v in rb["nssm"].items() if k != "fov_ambiguous"})   # (store runs only)
        assert _records_equal(ra, rb), (ra, rb)
    assert host[1] == dev[1]
    # compute_icp_with_cov ran (over the store in `dev`)
    assert any((r.get("nssm") or {}).get("n_guesses", 0) > 0 for r in dev[0])
    assert not all(_records_equal(ra, rb) for ra, rb in zip(dev[0], shipped[0])), "the chain changes nothing here"


def _sessions(S, K, rows=512, beams=256):
    from sonar_slam_amd.feature_extraction import oculus_bearings
    world = synth.world_structure(seed=2, n=8000)
    bearings = oculus_bearings(beams)
    frames = np.zeros((K, S, rows, beams), np.uint8)
    dr = np.zeros((S, K, 3))
    for s in range(S):
        t, d = synth.trajectory(n=K, step=1.7, turn=0.03 + 0.01 * (s % 4), start=(2.0 + 0.5 * s, 0.3 * s - 1.0, 0.02 * s),
                                seed=100 + s)
        dr[s] = d
        for k in range(K):
            frames[k, s] = synth.render_ping(world, t[k], bearings, rows=rows, seed=1000 * s + k)
    return frames, dr, bearings


def test_sessions_under_a_chain_equal_front_ends_on_a_store(ctx, shipped_cfar):
    """chained.SessionBatch with an IcpChain == replay.FrontEnd(icp_params=chain) on a store, session by session"""
    from sonar_slam_amd import chained
    from sonar_slam_amd.feature_extraction import FeatureExtraction, SonarPing
    from sonar_slam_amd.replay import FrontEnd, replay
    S, K, rows, beams = 4, 6, 512, 256
    frames, dr, bearings = _sessions(S, K, rows, beams)
    fe = FeatureExtraction(ctx)
    fe.Ntc, fe.Ngc, fe.Pfa, fe.rank, fe.alg, fe.threshold = 40, 10, 0.1, 10, "SOCA", 65
    fe.resolution, fe.outlier_filter_radius, fe.outlier_filter_min_points, fe.skip = 0.5, 1.0, 5, 1
    fe.configure()
    fe.generate_map_xy(SonarPing(frames[0, 0], bearings, 30.0 / rows))
    chain = R.chain("replay")
    sb = chained.SessionBatch(ctx, fe.geometry, shipped_cfar.params["SOCA"], "SOCA", 65, chain, S, K, dr)
    assert sb.kb.icp_params is chain.params
    for k in range(K):
        sb.upload_frames(k, frames[k])
    recs = [dict(r) for r in sb.run()]
    sb.icp_params = icp_config.shipped_params()
    shipped = [dict(r) for r in sb.run()]
    assert any(not np.array_equal(a["T"], b["T"]) for a, b in zip(recs[1:], shipped[1:])), "the chain changes nothing"
    n_success = 0
    for s in range(S):
        store = st.CloudStore(ctx, capacity_points=1 << 18, max_clouds=64)
        front = FrontEnd(ctx, icp_params=chain, keyframe_translation=1.5, keyframe_duration=0.5, store=store,
                         ssm_initialization=False, nssm_enable=False)
        pings = [SonarPing(frames[k, s], bearings, 30.0 / rows, ping_id=k) for k in range(K)]
        log, _, _ = replay(pings, np.arange(K, dtype=float), dr[s], fe, front)
        assert len(log) == K
        for k in range(K):
            r, a = recs[k], log[k]
            name = chained.STATUS_NAMES[r["status"][s]]
            assert name == a["status"], (s, k, name, a["status"])
            assert r["n_source"][s] == a["n_source"] and tuple(r["pose"][s]) == a["pose"]
            if k == 0:
                continue
            assert r["n_target"][s] == a["n_target"]
            if "transform" in a:
                assert tuple(r["transform"][s]) == a["transform"], (s, k)
            if "overlap" in a:
                assert r["overlap"][s] == a["overlap"]
            n_success += name == "SUCCESS"
        store.close()
    assert n_success >= S * (K - 1) - 3
    sb.free()


def test_farm_with_a_chain_equals_one_compute_jobs_call(ctx):
    """IcpFarm(chain) with two workers on one device and chunks of 7 (jobs that share a cloud land in different chunks,
    each of which filters it again) == one pcl.ICP.compute_jobs call with the chain"""
    from sonar_slam_amd import farm
    chain = R.chain("outliers")
    chain.reading = R.chain("filters").reading
    chain.reference = R.chain("filters").reference
    srcs, tgts, pairs, guesses = _jobs("shared")
    jobs = []
    for j, (a, b) in enumerate(pairs):
        jobs.append((srcs[a], tgts[b], [guesses[j]] + ([_noisy(guesses[j], np.random.default_rng(j), 0.3)] if j % 3 == 0 else [])))
    with farm.IcpFarm(chain, devices=[ctx.device, ctx.device], chunk=7) as f:
        out = f.run(jobs)
    # the whole table in one call
    icp = pcl.ICP(ctx)
    icp.setChain(chain)
    src_pool, tgt_pool, _, _, rows, gs = farm.pack_jobs(jobs)
    stt, T, it = icp.compute_jobs(np.concatenate(src_pool), np.concatenate(tgt_pool), np.asarray(rows, np.int32),
                                  np.stack(gs))
    statuses, k0 = [], 0
    for j, (msgs, Tf, itf) in enumerate(out):
        k = len(jobs[j][2])
        assert msgs == [L.ICP_STATUS_MESSAGES.get(int(x), "ICP failure %d" % x) for x in stt[k0:k0 + k]], j
        assert np.array_equal(Tf, T[k0:k0 + k]) and np.array_equal(itf, it[k0:k0 + k]), j
        statuses.extend(stt[k0:k0 + k].tolist())
        k0 += k
    assert L.ICP_BOUND in statuses and 0 in statuses
    # ... and a shipped farm gives other results on the same jobs
    with farm.IcpFarm(icp_config.shipped_params(), devices=[ctx.device]) as f:
        plain = f.run(jobs)
    assert any(not np.array_equal(a[1], b[1]) for a, b in zip(out, plain))
