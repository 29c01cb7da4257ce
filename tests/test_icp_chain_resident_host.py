"""CPU: ICP chains on the resident routes -- the IcpChain dict / pickle round trip a chain farm sends its workers, the
types ``store.CloudStore.icp``, ``replay.FrontEnd``, ``chained.SessionBatch`` and ``farm.IcpFarm`` accept and refuse,
the ctypes call each store route makes (the library mocked), and a chain farm of two worker processes on the CPU."""
import ctypes as C
import os
import pickle
import sys
import threading

import numpy as np
import pytest

from sonar_slam_amd import _lib as L
from sonar_slam_amd import icp_config
from sonar_slam_amd import store as st

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resident_chains as R  # noqa: E402

ALL = ("shipped",) + tuple(R.CHAINS)


@pytest.mark.parametrize("name", ALL)
def test_chain_dict_and_pickle_round_trips(name):
    chain = R.chain(name)
    d = chain.as_dict()
    back = icp_config.IcpChain.from_dict(d)
    assert back == chain and back.as_dict() == d
    assert icp_config.IcpChain.from_dict(pickle.loads(pickle.dumps(d))) == chain
    assert pickle.loads(pickle.dumps(d)) == d
    # plain values only: no ctypes object leaves the chain
    def plain(x):
        if isinstance(x, dict):
            return all(isinstance(k, str) and plain(v) for k, v in x.items())
        if isinstance(x, list):
            return all(plain(v) for v in x)
        return isinstance(x, (int, float, str))
    assert plain(d)
    # the rebuilt chain owns new structures, with the same bytes
    for a, b in zip(chain.reading + chain.reference, back.reading + back.reference):
        assert a is not b
        if isinstance(a, L.IcpDpf):
            assert bytes(a) == bytes(b)
        else:
            assert a == b
    assert bytes(back.params) == bytes(chain.params) and bytes(back.outliers) == bytes(chain.outliers)


def test_every_supported_module_survives_the_round_trip():
    text = """readingDataPointsFilters:
  - MaxDistDataPointsFilter: {dim: 0, maxDist: 12.5}
  - MinDistDataPointsFilter: {dim: -1, minDist: 0.75}
  - BoundingBoxDataPointsFilter: {xMin: -3.0, xMax: 4.0, yMin: -5.0, yMax: 6.0, removeInside: 1}
referenceDataPointsFilters:
  - OctreeGridDataPointsFilter: {maxSizeByNode: 0.3, samplingMethod: 3}
  - MaxDistDataPointsFilter: {dim: 1, maxDist: -2.0}
  - SurfaceNormalDataPointsFilter: {knn: 7}
matcher:
  KDTreeMatcher: {maxDist: 5.0}
outlierFilters:
  - NullOutlierFilter
  - MinDistOutlierFilter: {minDist: 0.1}
  - MedianDistOutlierFilter: {factor: 1.7}
  - TrimmedDistOutlierFilter: {ratio: 0.6}
errorMinimizer:
  PointToPlaneErrorMinimizer: {force2D: 1}
transformationCheckers:
  - DifferentialTransformationChecker: {minDiffRotErr: 0.002, minDiffTransErr: 0.02, smoothLength: 2}
  - BoundTransformationChecker: {maxRotationNorm: 0.3, maxTranslationNorm: 1.5}
  - CounterTransformationChecker: {maxIterationCount: 17}
"""
    chain = icp_config.parse_icp_chain(text)
    assert len(chain.reading) == 3 and len(chain.reference) == 3 and chain.outliers.bound_order == 2
    back = icp_config.IcpChain.from_dict(pickle.loads(pickle.dumps(chain.as_dict())))
    assert back == chain and repr(back) == repr(chain)
    assert isinstance(back.reference[-1], icp_config.SurfaceNormalStage) and back.reference[-1].knn == 7


def test_chain_equality_sees_every_part():
    base = R.chain("replay")
    assert base == R.chain("replay") and not (base != R.chain("replay"))
    for change in (lambda c: setattr(c.params, "max_iter", 41),
                   lambda c: c.reading.pop(),
                   lambda c: c.reference[0].f.__setitem__(0, 0.71),
                   lambda c: setattr(c.outliers, "median_factor", 3.5)):
        other = R.chain("replay")
        change(other)
        assert other != base
    assert base != base.params and base != base.as_dict()
    with pytest.raises(TypeError):
        hash(base)


# ---- store.CloudStore.icp with the library mocked ----
class _Lib(object):
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


class _Ctx(object):
    def __init__(self):
        self.lib, self.handle, self.lock = _Lib(), C.c_void_p(1), threading.RLock()

    def _check(self, rc):
        assert rc == 0


def _store():
    s = st.CloudStore.__new__(st.CloudStore)
    s.ctx, s.handle = _Ctx(), C.c_void_p(2)
    return s


def _pointee(arg):
    return arg._obj if arg is not None else None


def test_store_icp_routes_by_chain():
    pairs, guesses = [(0, 1), (0, 2)], np.stack([np.eye(3)] * 2)
    # IcpParams: today's call
    s = _store()
    p = icp_config.shipped_params()
    s.icp(p, pairs, guesses)
    (name, args), = s.ctx.lib.calls
    assert name == "sfe_icp_store_compute" and _pointee(args[1]) is p
    # a chain without modules: the same call, with its params
    s = _store()
    chain = R.chain("shipped")
    s.icp(chain, pairs, guesses)
    (name, args), = s.ctx.lib.calls
    assert name == "sfe_icp_store_compute" and _pointee(args[1]) is chain.params
    # filters and outlier modules: the chain entry point with the device stages and the outliers
    for cname in ("filters", "outliers", "plane", "empty", "replay"):
        s = _store()
        chain = R.chain(cname)
        s.icp(chain, pairs, guesses)
        (name, args), = s.ctx.lib.calls
        assert name == "sfe_icp_store_compute_chain_ext", cname
        assert _pointee(args[1]) is chain.params
        assert (_pointee(args[2]) is chain.outliers) == chain.outliers.any()
        assert args[2] is None or chain.outliers.any()
        dev_rd = [x for x in chain.reading if isinstance(x, L.IcpDpf)]
        dev_rf = [x for x in chain.reference if isinstance(x, L.IcpDpf)]
        assert args[4] == len(dev_rd) and args[6] == len(dev_rf)
        for arr, want in ((args[3], dev_rd), (args[5], dev_rf)):
            assert (arr is None) == (not want)
            assert [bytes(x) for x in (arr or [])] == [bytes(x) for x in want]
        assert args[7] is s.handle and args[10] == 2


@pytest.mark.parametrize("bad", [None, {"max_iter": 3}, "icp.yaml", 3])
def test_store_icp_refuses_other_types(bad):
    s = _store()
    with pytest.raises(TypeError, match="IcpParams or an icp_config.IcpChain"):
        s.icp(bad, [(0, 1)], [np.eye(3)])
    assert s.ctx.lib.calls == []


# ---- replay.FrontEnd ----
class _FakeStore(object):
    def __init__(self):
        self.seen = []

    def icp(self, params_or_chain, pairs, guesses):
        self.seen.append(params_or_chain)
        n = len(pairs)
        T = np.stack([np.eye(3, dtype=np.float32)] * n)
        T[:, :2, 2] = np.random.default_rng(n).normal(0, 0.1, (n, 2))
        return T, np.zeros(n, np.int32), np.ones(n, np.int32)


def test_front_end_takes_a_chain_and_hands_the_installed_one_to_the_store(tmp_path):
    from sonar_slam_amd.pose2 import Pose2
    from sonar_slam_amd.replay import CloudRef, FrontEnd
    chain = R.chain("filters")
    fe = FrontEnd(icp_params=chain)
    assert fe.icp.chain is chain and fe.icp.params is chain.params
    fe = FrontEnd()
    assert fe.icp.params.as_dict() == icp_config.shipped_params().as_dict()
    fe.store = _FakeStore()
    src, tgt = CloudRef(0, 100), CloudRef(1, 100)
    fe.compute_icp(src, tgt, Pose2(0.0, 0.0, 0.0))
    assert not fe.store.seen[-1].has_modules()
    # a chain loaded after construction reaches both store call sites
    path = tmp_path / "icp.yaml"
    path.write_text(R.CHAINS["outliers"])
    fe.icp.loadFromYaml(str(path))
    fe.compute_icp(src, tgt, Pose2(0.0, 0.0, 0.0))
    assert fe.store.seen[-1] == R.chain("outliers")
    fe.compute_icp_with_cov(src, tgt, [Pose2(0.0, 0.0, 0.0)] * 6)
    assert fe.store.seen[-1] == R.chain("outliers")
    fe.icp.setChain(R.chain("empty"))
    fe.compute_icp(src, tgt, Pose2(0.0, 0.0, 0.0))
    assert fe.store.seen[-1] is fe.icp.chain
    # ICP.params replaced by hand: pcl.ICP would run it with the chain's modules, so does the store
    fe.icp.params = icp_config.shipped_params(max_iter=7)
    fe.compute_icp(src, tgt, Pose2(0.0, 0.0, 0.0))
    got = fe.store.seen[-1]
    assert got.params is fe.icp.params and got.reading == fe.icp.chain.reading
    # ... and an empty chain is still an error, on the store path as well
    fe.icp = type(fe.icp)()
    with pytest.raises(RuntimeError, match="before loadFromYaml / setParams"):
        fe.compute_icp(src, tgt, Pose2(0.0, 0.0, 0.0))


@pytest.mark.parametrize("bad", [{"max_iter": 3}, "icp.yaml"])
def test_front_end_refuses_other_types(bad):
    from sonar_slam_amd.replay import FrontEnd
    with pytest.raises(TypeError, match="IcpParams or an icp_config.IcpChain"):
        FrontEnd(icp_params=bad)


# ---- chained.SessionBatch ----
def test_session_batch_icp_params_takes_a_chain():
    from sonar_slam_amd import chained
    sb = chained.SessionBatch.__new__(chained.SessionBatch)
    chain = R.chain("replay")
    sb.icp_params = chain
    assert sb.icp_params is chain and sb._kb_params() is chain.params
    p = icp_config.shipped_params()
    sb.icp_params = p                       # what tools/bench_legs.py does between runs
    assert sb.icp_params is p and sb._kb_params() is p
    for bad in (None, p.as_dict(), "icp.yaml"):
        with pytest.raises(TypeError, match="IcpParams or an icp_config.IcpChain"):
            sb.icp_params = bad
    assert sb.icp_params is p


# ---- farm.IcpFarm ----
@pytest.mark.parametrize("bad", [None, {"max_iter": 3}, "icp.yaml"])
def test_farm_refuses_other_types(bad):
    from sonar_slam_amd import farm
    with pytest.raises(TypeError, match="IcpParams or an icp_config.IcpChain"):
        farm.IcpFarm(bad, devices=[0])


def test_farm_hands_the_workers_the_right_dict():
    from sonar_slam_amd import farm
    p = icp_config.shipped_params()
    chain = R.chain("outliers")
    assert not farm.is_chain_dict(p.as_dict()) and farm.is_chain_dict(chain.as_dict())
    assert farm.IcpFarm(p, devices=[0]).params is p and farm.IcpFarm(chain, devices=[0]).params is chain


def _mirrored(c):
    return np.c_[-np.abs(c[:, 0]) - 2.0, c[:, 1]].astype(np.float32)


def _farm_jobs():
    from sonar_slam_amd import synth
    pairs = [synth.scan_pair(seed=60 + s, n_src=140 + 20 * s, n_tgt=150) for s in range(3)]
    far = _mirrored(pairs[0][0])                                           # left empty by the 'empty' chain
    rng = np.random.default_rng(4)
    jobs = []
    for j in range(9):
        s, t, g, _ = pairs[j % 3]
        if j == 4:
            s = far
        jobs.append((s, t, [(g @ synth.pose_matrix(*rng.normal(0, [0.3, 0.3, 0.06] if k else [0.05, 0.05, 0.01])))
                            .astype(np.float32) for k in range(1 + j % 2)]))
    return jobs


@pytest.mark.parametrize("name", ["filters", "outliers", "empty"])
def test_two_worker_chain_farm_on_the_cpu(name):
    """world size 2: the chain reaches both workers intact (the CPU backend rebuilds it from the dict), results come back
    in job order and equal the backend's computation in this process; they differ from the shipped chain's"""
    import oracle
    from sonar_slam_amd import farm
    import farm_chain_backend as B
    chain = R.chain(name)
    jobs = _farm_jobs()
    with farm.IcpFarm(chain, devices=[0, 1], chunk=4, _backend="farm_chain_backend:oracle_chain_compute") as f:
        out = f.run(jobs)
        assert len(set(w.name for w in f._workers)) == 2
    assert len(out) == len(jobs)
    differs, statuses = False, []
    for (s, t, gs), (msgs, T, it) in zip(jobs, out):
        assert len(msgs) == len(gs) == len(T) == len(it)
        for g, m, Tj, i in zip(gs, msgs, T, it):
            sw, Tw, iw = B.chain_job(chain, s, t, g)
            assert m == L.ICP_STATUS_MESSAGES[sw] and i == iw and np.array_equal(Tj, Tw)
            so, To, io = oracle.icp(s, t, g, oracle.IcpParams(precision=1, **icp_config.shipped_params().as_dict()))
            differs |= (sw, iw) != (so, io) or not np.array_equal(Tw, To)
            statuses.append(sw)
    assert differs, "the chain changes nothing on these jobs"
    if name == "empty":
        assert B.DPF_EMPTY in statuses
    if name == "outliers":
        assert L.ICP_BOUND in statuses


def test_params_farm_still_hands_params_as_dict_to_the_oracle_backend():
    import oracle
    from sonar_slam_amd import farm
    p = icp_config.shipped_params()
    jobs = _farm_jobs()[:4]
    with farm.IcpFarm(p, devices=[0, 1], chunk=3, _backend="farm_backend:oracle_compute") as f:
        out = f.run(jobs)
    for (s, t, gs), (msgs, T, it) in zip(jobs, out):
        for g, m, Tj, i in zip(gs, msgs, T, it):
            so, To, io = oracle.icp(s, t, g, oracle.IcpParams(precision=1, **p.as_dict()))
            assert m == oracle.ICP_STATUS_MESSAGES[so] and i == io and np.array_equal(Tj, To)
    # ... and the chain backend refuses a params dict: a farm never sends one where the other belongs
    with pytest.raises(RuntimeError, match="IcpChain.as_dict"):
        with farm.IcpFarm(p, devices=[0], _backend="farm_chain_backend:oracle_chain_compute") as f:
            f.run(jobs[:1])
