"""chained.SessionBatch(nssm_enable=True): the loop-closure search (slam.py:839-1087) of every session in lock-step, one device
call per stage over the sessions still searching -- record for record, bit for bit, what replay.FrontEnd(store=...) records on
the same pings; and the many-job store entry points it runs on against their single-job forms, job by job."""
import copy

import numpy as np
import pytest

from test_global_init import _product_fe, _replay_session, _same, _session

K, ROWS = 15, 256
NSSM = dict(nssm_enable=True, nssm_min_points=30, mcd_random_state=0)


def _sessions(n):
    """the recipe of test_front_end_loop_closure_search_equals_the_oracle_chain, a different seed and start per session"""
    return [_session(K, rows=ROWS, step=1.7, turn=2 * np.pi / 13, seed=21 + 4 * s, n_world=9000,
                     start=(20.0 - 1.5 * s, 0.8 * s, 0.1 * s)) for s in range(n)]


def _batch(ctx, shipped_cfar, pings, dr, **kw):
    from sonar_slam_amd import chained, icp_config
    from sonar_slam_amd.feature_extraction import SonarPing, oculus_bearings
    fe = _product_fe(ctx)
    fe.generate_map_xy(SonarPing(pings[0][0], oculus_bearings(pings.shape[-1]), 30.0 / ROWS))
    sb = chained.SessionBatch(ctx, fe.geometry, shipped_cfar.params["SOCA"], "SOCA", 65, icp_config.shipped_params(), len(pings),
                              K, dr, ssm_min_points=20, initialization=True, **kw)
    for k in range(K):
        sb.upload_frames(k, pings[:, k])
    return sb


def _front(ctx, sess, **kw):
    from sonar_slam_amd import store as st
    store = st.CloudStore(ctx, capacity_points=1 << 18, max_clouds=256)
    front, log = _replay_session(ctx, sess[0], sess[4], sess[2], ROWS, store, ssm_min_points=20, **kw)
    assert len(log) == K and len(store) == K
    store.close()
    return log, [f for f in front.backend.factors if f[0] == "loop"]


def _same_nssm(a, b, skip=()):
    assert (a is None) == (b is None), (a, b)
    if a is None:
        return
    assert set(a) - set(skip) == set(b) - set(skip), set(a) ^ set(b)
    for key in a:
        if key not in skip:
            assert type(a[key]) is type(b[key]) or key in ("sample_transforms", "cov"), (key, type(a[key]), type(b[key]))
            assert _same(a[key], b[key]), (key, a[key], b[key])


def _same_loops(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x[:3] == y[:3]
        assert (x[3].x(), x[3].y(), x[3].theta()) == (y[3].x(), y[3].y(), y[3].theta())
        assert (x[4] is None) == (y[4] is None) and (x[4] is None or np.array_equal(x[4], y[4]))


def _compare(recs, batch_loops, s, log, loops, skip=()):
    """session s of the batch's records against FrontEnd's log: scan match, search record, loop factors -> the search statuses"""
    from sonar_slam_amd import chained
    statuses = set()
    for k in range(K):
        r, a = recs[k], log[k]
        assert chained.STATUS_NAMES[r["status"][s]] == a["status"] and tuple(r["pose"][s]) == a["pose"], (s, k)
        if "transform" in a:
            assert tuple(r["transform"][s]) == a["transform"] and r["overlap"][s] == a["overlap"]
        if "init_x" in a:
            assert tuple(r["init_x"][s]) == a["init_x"] and r["init_cost"][s] == a["init_cost"]
        _same_nssm(r["nssm"][s], a.get("nssm"), skip)
        if r["nssm"][s] is not None:
            statuses.add(r["nssm"][s]["status"])
    _same_loops(batch_loops[s], loops)
    return statuses


@pytest.fixture(scope="module")
def lockstep(ctx, shipped_cfar):
    """S = 3 closed-loop sessions + one whose pings hold nothing (it diverges at every gate), one batch"""
    sess = _sessions(3)
    pings = np.stack([x[0] for x in sess] + [np.zeros_like(sess[0][0])])
    dr = np.stack([x[2] for x in sess] + [sess[0][2]])
    sb = _batch(ctx, shipped_cfar, pings, dr, **NSSM)
    sb.warm_up()
    recs = sb.run()
    out = dict(sess=sess, pings=pings, dr=dr, recs=copy.deepcopy(recs), loops=copy.deepcopy(sb.loops), n_store=len(sb.store),
               fronts=[_front(ctx, x, **NSSM) for x in sess])
    sb.free()
    return out


@pytest.mark.gpu
def test_lock_step_loop_closure_search_equals_front_end(lockstep):
    """every step, every session: scan match, search record (fov_ambiguous, init_replayed, sample_transforms, cov included) and
    loop factors of replay.FrontEnd; every search cloud dropped at the end of its step"""
    recs = lockstep["recs"]
    assert lockstep["n_store"] == 4 * K
    statuses = set()
    for s in range(3):
        log, loops = lockstep["fronts"][s]
        statuses |= _compare(recs, lockstep["loops"], s, log, loops)
    assert "SUCCESS" in statuses and len(statuses - {"SUCCESS"}) >= 2, statuses
    assert sum(len(lockstep["loops"][s]) for s in range(3)) >= 1
    assert all(recs[k]["nssm"] == [None] * 4 for k in range(7))


@pytest.mark.gpu
def test_a_session_without_points_leaves_the_others_unchanged(lockstep):
    """the empty session fails the search's first gate at every step; its neighbours' records are FrontEnd's (above) -- and
    the same whether it is in the batch or not"""
    for k in range(7, K):
        r = lockstep["recs"][k]["nssm"][3]
        assert r == {"source_key": k, "n_source": 0, "status": "NOT_ENOUGH_POINTS"}, r
    assert lockstep["loops"][3] == []


@pytest.mark.gpu
def test_lock_step_variants_equal_front_end(ctx, shipped_cfar, lockstep):
    """nssm_initialization=False, nssm_cov_samples=0: FrontEnd with the same settings; shgo_replay=False and forced fallbacks
    (the replay says FALLBACK, the device gate says ambiguous for some sessions): the records of the replayed run"""
    from sonar_slam_amd import shgo_fast
    sess, pings, dr = lockstep["sess"][:2], lockstep["pings"][:2], lockstep["dr"][:2]
    for kw in (dict(nssm_initialization=False), dict(nssm_cov_samples=0)):
        sb = _batch(ctx, shipped_cfar, pings, dr, **NSSM, **kw)
        recs = sb.run()
        n_search = 0
        for s in range(2):
            log, loops = _front(ctx, sess[s], **NSSM, **kw)
            _compare(recs, sb.loops, s, log, loops)
            n_search += sum(recs[k]["nssm"][s] is not None and "icp" in recs[k]["nssm"][s] for k in range(K))
        assert n_search >= 1 and len(sb.store) == 2 * K
        sb.free()
    # scipy.optimize.shgo itself for every search
    sb = _batch(ctx, shipped_cfar, pings, dr, shgo_replay=False, **NSSM)
    recs = sb.run()
    for s in range(2):
        log, loops = lockstep["fronts"][s]
        _compare(recs, sb.loops, s, log, loops, skip=("init_replayed",))
        assert all(recs[k]["nssm"][s] is None or not recs[k]["nssm"][s].get("init_replayed", False) for k in range(K))
    sb.free()
    # forced: every other replay reports FALLBACK (scipy.optimize.shgo takes those searches), and the device gate reports
    # session 1 ambiguous at every step (numpy decides its selection)
    sb = _batch(ctx, shipped_cfar, pings, dr, **NSSM)
    calls = {"n": 0, "fell": 0, "amb": 0}

    def replay(*a):
        calls["n"] += 1
        out = shgo_fast.replay_multi(*a)
        if calls["n"] % 2 == 0 and out[0] != shgo_fast.FALLBACK:
            calls["fell"] += 1
            return (shgo_fast.FALLBACK, None, None, None, None)
        return out
    real_fov = sb.store.fov_select_many

    def fov(*a, **k):
        hist, n_sel, n_amb = real_fov(*a, **k)
        if len(n_amb) > 1:
            n_amb = n_amb.copy()
            n_amb[1] += 1
            calls["amb"] += 1
        return hist, n_sel, n_amb
    sb._replay_multi = replay
    sb.store.fov_select_many = fov
    recs = sb.run()
    assert calls["fell"] >= 1 and calls["amb"] >= 1
    for s in range(2):
        log, loops = lockstep["fronts"][s]
        _compare(recs, sb.loops, s, log, loops, skip=("init_replayed", "fov_ambiguous"))
    sb.free()


@pytest.mark.gpu
def test_many_job_store_entry_points_equal_the_single_job_calls(ctx):
    """get_points_keys_many / fov_select_many / compact_selected_many / match_keys_many == the single-job call, job by job, bit
    for bit: an empty job, a job with nothing selected, jobs of very different sizes, a keyed target beyond the resident
    filter's capacity (65 536 points)"""
    from sonar_slam_amd import store as st
    from sonar_slam_amd.pose2 import Pose2
    rng = np.random.default_rng(5)
    s = st.CloudStore(ctx, capacity_points=1 << 20, max_clouds=256)
    sizes = (9000, 0, 9500, 8000, 1, 9000, 9000, 9000, 9000, 9200, 40, 300)
    clouds = [np.c_[rng.uniform(1, 29, n), rng.uniform(-20, 20, n)].astype(np.float32) for n in sizes]
    hs = np.array([s.put(c) for c in clouds], np.int32)
    poses = [Pose2(*q) for q in np.c_[np.cumsum(rng.uniform(1, 3, len(sizes))), rng.normal(0, 2, len(sizes)),
                                      rng.normal(0, 0.4, len(sizes))]]
    T6 = np.array([st.pose_T6(p) for p in poses])
    jobs = [list(range(10)), [1], [10, 11], [4], [11, 0, 3], []]          # > 65 536 points, empty, small, one point, mixed, none
    assert sum(sizes[i] for i in jobs[0]) > 65536
    keys = [[3 + i for i in j] for j in jobs]
    for flags in (0, st.F32_POINTS):
        one = [s.get_points_keys(hs[j], T6[j], kk, 0.5, flags=flags) for j, kk in zip(jobs, keys)]
        many = s.get_points_keys_many([hs[j] for j in jobs], [T6[j] for j in jobs], keys, 0.5, flags=flags)
        for a, b in zip(one, many):
            assert np.array_equal(s.read(a).view(np.uint32), s.read(b).view(np.uint32)) and np.array_equal(s.read_keys(a), s.read_keys(b))
    assert s.counts(many)[1] == 0 and s.counts(many)[0] > 3000
    # the gate: every job its own frames; job 2 selects nothing
    frames = [[Pose2(8.0, 1.0, 0.3), Pose2(14.0, -2.0, -0.4)], [Pose2(3.0, 0.0, 1.2)], [Pose2(-500.0, 0.0, 0.0)], [Pose2(5.0, 1.0, 0.1)],
              [Pose2(9.0, 0.0, 0.0), Pose2(2.0, 2.0, 2.0), Pose2(12.0, -3.0, -1.0)], []]
    Tinv = [[st.pose_T6(f.inverse()) for f in fr] for fr in frames]
    rb = [[12.0, 9.5], [30.0], [10.0], [20.0], [11.0, 8.0, 30.0], []]
    bb = [[1.2, 0.7], [0.4], [1.0], [1.1], [0.5, 0.9, 1.3], []]
    want = [s.fov_select(h, t, r, b, 16) for h, t, r, b in zip(many, Tinv, rb, bb)]
    hist, n_sel, n_amb = s.fov_select_many(many, Tinv, rb, bb, 16)
    for j, (h1, n1, a1) in enumerate(want):
        assert np.array_equal(hist[j], h1) and n_sel[j] == n1 and n_amb[j] == a1, j
    assert n_sel[2] == 0 and n_sel[0] > 100 and n_sel[1] == 0
    comp1 = [s.compact_selected(h) for h in many]             # (every cloud keeps its own selection)
    comp = s.compact_selected_many(many)
    for a, b in zip(comp1, comp):
        assert np.array_equal(s.read(a).view(np.uint32), s.read(b).view(np.uint32)) and np.array_equal(s.read_keys(a), s.read_keys(b))
    # matches of moved sources against the keyed targets: sources of very different sizes, one empty
    srcs = [s.put(clouds[i][::3]) for i in (5, 1, 10, 4, 7, 0)]
    est = [st.pose_T6(Pose2(*rng.normal(0, [0.3, 0.3, 0.02]))) for _ in srcs]
    for flags in (0, st.F32_POINTS):
        want = [s.match_keys(a, t, b, 0.5, 16, flags=flags) for a, t, b in zip(srcs, est, comp)]
        h2, ov = s.match_keys_many(srcs, est, comp, 0.5, 16, flags=flags)
        for j, (h1, o1) in enumerate(want):
            assert np.array_equal(h2[j], h1) and ov[j] == o1, j
    assert ov[0] > 50 and ov[1] == 0
    s.close()
