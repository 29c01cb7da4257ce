"""GPU: consecutive ICP batches on one context with the preparation on the side stream (sfe_icp_set_tuning bit 3).

What the target preparation writes and the loop kernels read (job tables, sorted targets, permutations, normals, means,
sort keys, strip tables, witness grids) exists in two generations, used in turn: the preparation of a batch waits for
the loop kernels of the batch two back, not for those of the batch before, which may still be running.  Every test
enqueues its batches back to back without a synchronisation in between (all device buffers are allocated and uploaded
first: an upload synchronises) and holds every batch bit for bit against the same batch computed alone, on a fresh
context, without bit 3.

What these tests can and cannot see: the batches have different targets, so a loop kernel that reads the wrong generation,
or a generation that the wrong preparation wrote, changes a result every time.  A missing wait -- a preparation that
overwrites a generation while a loop kernel still reads it, a block freed under a pending kernel -- only changes a result
if the two really overlap, and batches this small are over in tens of microseconds: the loop kernel has most likely
drained before the later preparation starts, so such a bug would most likely still pass here.  That every preparation
waits for the right loop kernels is shown by the model in tests/host/icp_gen_check.cpp (tests/test_icp_gen_rules.py), which
runs the same rules (sfe_icp_gen.h) over every sequence of batches, not by timing.

Shapes: the smallest that reach every preparation and loop kernel.  A call of a few jobs (the `mixed` batches):
  40 x 40, 300 x 300    the exhaustive one-wave kernel (point-to-plane: its normals come from the 256-thread preparation)
  300 x 1500            256-thread preparation, four-wave loop kernel
  1500 x 1500           256-thread preparation (its capacity is 2048 points), 1024-thread loop kernel
  2100 x 2100           the smallest class above it: 1024-thread preparation and loop kernel
The one-wave preparation and loop kernel are only chosen when a call holds at least 2 x CUs jobs that fit them, and
clouds of that size go to the exhaustive kernel first: test_one_wave_tier brings 2 x CUs + 4 jobs of about 300 points
and switches the exhaustive kernel off.  Jobs shared by several workgroups (8192 queries on a target beyond 8192
points) keep ONE copy of their own scratch and the wait for the newest loop kernel: test_shared_jobs_keep_the_old_wait.
Both minimisers, three to five iterations."""
import numpy as np
import pytest

from sonar_slam_amd import _lib as L
from sonar_slam_amd import icp_config, synth
from sonar_slam_amd.pipeline import ScanMatchBatch

pytestmark = pytest.mark.gpu

CHAINS = {"p2p": dict(max_iter=4), "p2plane": dict(minimizer=1, max_iter=5, use_diff_checker=0)}
MIXED = [(40, 40), (40, 40), (300, 300), (300, 300), (300, 1500), (1500, 1500), (1500, 1500), (2100, 2100), (2100, 2100)]
MIXED_ROUTES = [L.ICP_ROUTE_TINY] * 4 + [L.ICP_ROUTE_T1] + [L.ICP_ROUTE_Q] * 4
SMALL = [(40, 40), (300, 1500), (1500, 1500), (2100, 2100)]


class Spec(object):
    """the host side of one batch: clouds, job table, guesses, launcher knobs"""

    def __init__(self, seed, sizes, jobs=None, guesses=None, knobs=None):
        pairs = [synth.scan_pair(seed=seed + i, n_src=a, n_tgt=b) for i, (a, b) in enumerate(sizes)]
        self.srcs, self.tgts = [q[0] for q in pairs], [q[1] for q in pairs]
        self.jobs = jobs if jobs is not None else [(j, j) for j in range(len(pairs))]
        self.gs = guesses if guesses is not None else [pairs[a][2] for a, _ in self.jobs]
        self.knobs = knobs or {}
        self.alone = {}       # chain -> (T, status, iters, routes) of the batch alone: computed once, never changed


def _spread(seed, g, n):
    rng = np.random.default_rng(seed)
    return [g] + [(g.astype(np.float64) @ synth.pose_matrix(*rng.normal(0, [0.1, 0.1, 0.01]))).astype(np.float32)
                  for _ in range(n - 1)]


def _results(b):
    r = b.results()
    return r["T"], r["status"], r["iters"]


def _alone(spec, chain):
    """the batch alone on a fresh context, bit 3 clear"""
    if chain not in spec.alone:
        c = L.Context(0)
        try:
            b = ScanMatchBatch(c, icp_config.shipped_params(**CHAINS[chain]), spec.srcs, spec.tgts, spec.jobs, spec.gs)
            with c.tuning(**spec.knobs):
                b.run()
            routes = list(c.icp_routes(b.n))
            spec.alone[chain] = _results(b) + (routes,)
            b.free()
        finally:
            c.close()
    return spec.alone[chain]


def _back_to_back(chain, specs, bits):
    """the batches of `specs` enqueued one behind the other on ONE fresh context, batch i under sfe_icp_set_tuning(bits[i]),
    nothing synchronised between the first and the last call; every batch against itself alone"""
    p = icp_config.shipped_params(**CHAINS[chain])
    want = [_alone(s, chain) for s in specs]
    c = L.Context(0)
    try:
        batches = [ScanMatchBatch(c, p, s.srcs, s.tgts, s.jobs, s.gs) for s in specs]
        c.sync()
        for b, s, bit in zip(batches, specs, bits):
            c._check(c.lib.sfe_icp_set_tuning(c.handle, bit))
            with c.tuning(**s.knobs):
                b.run()
        got = [_results(b) for b in batches]
        for b in batches:
            b.free()
    finally:
        c.close()
    for i, (g, w) in enumerate(zip(got, want)):
        for k, name in enumerate(("T", "status", "iters")):
            assert np.array_equal(g[k], w[k], equal_nan=True), (chain, "batch %d of %d" % (i, len(specs)), name, np.flatnonzero(
                (g[k] != w[k]).reshape(len(w[1]), -1).any(axis=1))[:10])
    return want


@pytest.fixture(scope="module")
def abc():
    return [Spec(7100, MIXED), Spec(7200, MIXED), Spec(7300, MIXED)]


@pytest.fixture(scope="module")
def small():
    return [Spec(7400 + 10 * i, SMALL) for i in range(3)]


@pytest.mark.parametrize("chain", list(CHAINS))
def test_three_batches_back_to_back(abc, chain):
    """A, B, C with different clouds: B's preparation may run while A's loop kernels do (other generation), C's waits
    for A's loop kernels (same generation)"""
    want = _back_to_back(chain, abc, [8, 8, 8])
    for w in want:
        assert w[3] == MIXED_ROUTES, w[3]
        assert (w[1][4:] == 0).all(), w[1]


@pytest.mark.parametrize("chain", list(CHAINS))
def test_scratch_grows_and_shrinks_between_batches(abc, small, chain):
    """small, large, small, twice as large, large, small: the slots of generation 1 grow at the fourth batch and those of
    generation 0 at the fifth, each while the batch before may be pending (a slot that grows frees its block); the
    batches behind them are smaller than what the slots hold"""
    big = Spec(7500, MIXED + MIXED)
    _back_to_back(chain, [small[0], abc[0], small[1], big, abc[1], small[2]], [8] * 6)


@pytest.mark.parametrize("chain", list(CHAINS))
@pytest.mark.parametrize("order", ["side_first", "side_last"])
def test_bit_3_changes_between_batches(abc, chain, order):
    """A, B with bit 3, then C without it -- and C without it, then A, B with it -- no synchronisation where the bit
    changes: the single-generation batch is behind both generations' loop kernels, and the side stream's first
    preparation waits for the loop kernels of the batch without the bit"""
    if order == "side_first":
        _back_to_back(chain, abc, [8, 8, 0])
    else:
        _back_to_back(chain, [abc[2], abc[0], abc[1]], [0, 8, 8])


@pytest.mark.parametrize("chain", list(CHAINS))
def test_many_guesses_on_one_pair(chain):
    """eight guesses on one pair: one preparation serves the eight jobs of a batch; two such batches (a 256-thread and a
    1024-thread preparation) behind each other, and the first once more"""
    specs = []
    for i, n in enumerate((1500, 2100)):
        g = synth.scan_pair(seed=7600 + i, n_src=n, n_tgt=n)[2]
        specs.append(Spec(7600 + i, [(n, n)], jobs=[(0, 0)] * 8, guesses=_spread(76 + i, g, 8)))
    want = _back_to_back(chain, specs + specs[:1], [8, 8, 8])
    assert all(w[3] == [L.ICP_ROUTE_Q] * 8 for w in want), [w[3] for w in want]


@pytest.mark.parametrize("chain", list(CHAINS))
def test_one_wave_tier(ctx, chain):
    """2 x CUs + 4 jobs of about 300 points on six pairs, the exhaustive kernel off: the one-wave preparation and loop
    kernels, three batches"""
    n = 2 * ctx.n_cu + 4
    sizes = [(300, 300), (290, 310), (384, 512), (310, 290), (64, 300), (300, 65)]
    specs = []
    for k in range(3):
        base = Spec(7700 + 10 * k, sizes)
        jobs = [(j % len(sizes), j % len(sizes)) for j in range(n)]
        gs = []
        for i in range(len(sizes)):
            gs.append(_spread(770 + 10 * k + i, base.gs[i], (n + len(sizes) - 1) // len(sizes)))
        specs.append(Spec(7700 + 10 * k, sizes, jobs=jobs, guesses=[gs[j % len(sizes)][j // len(sizes)] for j in range(n)],
                          knobs=dict(sw_tiny=0)))
    want = _back_to_back(chain, specs, [8, 8, 8])
    assert all(w[3] == [L.ICP_ROUTE_T0] * n for w in want), [sorted(set(w[3])) for w in want]


@pytest.mark.parametrize("chain", list(CHAINS))
def test_shared_jobs_keep_the_old_wait(small, chain):
    """8192 queries on a target of 8193 points, alone in its call: the smallest job that is shared by several workgroups
    (sweep_batch: n_tgt > 8192 and n_src >= sw_multi_min_src = 8192).  Its shares must be resident together and its
    gathered clouds and sync areas exist once: the preparation behind it waits for its loop kernel, and its own
    preparation for every loop kernel before it.  Shared, small, shared, small."""
    shared = [Spec(7800 + i, [(8192, 8193)]) for i in range(2)]
    want = _back_to_back(chain, [shared[0], small[0], shared[1], small[1]], [8] * 4)
    assert want[0][3] == [L.ICP_ROUTE_SPLIT] and want[2][3] == [L.ICP_ROUTE_SPLIT], (want[0][3], want[2][3])
    assert want[0][1][0] == 0 and want[2][1][0] == 0, (want[0][1], want[2][1])
