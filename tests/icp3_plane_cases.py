"""The inputs of tests/test_gpu_icp3_plane.py, built here so that tests/test_icp3_plane_host.py can hold every one of them
to its conditions on the CPU -- the reference with its sums reversed, and with its normals moved by an ulp, lands on itself;
the clouds whose normals are compared have an eigen-gap; the cases built for a tie, a status or a stop have it -- and so that
both files share one reference result per job (``ref``, cached).  A job is (source N x 3, target M x 3, guess 4 x 4,
IcpParams with minimizer 2).  Coordinates stay within +-4 m.  Test infrastructure only."""
import functools

import numpy as np

from sonar_slam_amd import icp_config

import icp3_cases as C3
import icp3_plane_ref as R

f32 = np.float32
THREADS = C3.THREADS    # queries per pass of the job kernel's workgroup
TILE = C3.TILE          # target points resident in the job kernel's LDS
NTILE = 2048            # N3_TILE: points per LDS tile of the normals kernel
LANES = 256             # threads of a normals workgroup
GAP = 1e-3              # a normal is compared only where (l2 - l1) / l3 of its neighbourhood is at least this


def params(**kw):
    kw.setdefault("minimizer", 2)
    return icp_config.shipped_params(**kw)


# ---- scenes ----
def corner(rng, n, noise=0.005, walls=(0, 1, 2)):
    """n points on the faces x = -1.5, y = -1.5, z = -1 (those of ``walls``) of a box corner, 3 x 3 x 2 m, noisy"""
    w = np.asarray(walls)[rng.integers(0, len(walls), n)]
    u = rng.uniform(0, 1, (n, 3)) * np.array([3.0, 3.0, 2.0])
    u[np.arange(n), w] = 0.0
    return u - np.array([1.5, 1.5, 1.0]) + rng.normal(0, noise, (n, 3))


def pair(seed, ns, nt, noise=0.005, truth=C3.TRUTH, guess=C3.GUESS, walls=(0, 1, 2)):
    """-> (source, target, guess): target and source sampled independently on the same corner; the source is seen from a
    frame that ``truth`` maps onto the target's"""
    rng = np.random.default_rng(seed)
    tgt = corner(rng, nt, noise, walls)
    src = C3.apply(np.linalg.inv(truth), corner(rng, ns, noise, walls))
    return src.astype(f32), tgt.astype(f32), np.asarray(guess, f32)


def source_count_jobs():
    return [pair(1100 + ns, ns, 300) + (params(),) for ns in (1, 64, THREADS - 1, THREADS, THREADS + 1)]


def target_count_jobs():
    return [pair(1200 + k, 200, nt) + (params(),) for k, nt in enumerate((TILE - 1, TILE, TILE + 1, 2 * TILE + 1))]


def subset_job(knn, seed=1300, ns=150, nt=400):
    """a source that is a subset of the target under the identity guess: every kept pair has p == q to the bit, so e = 0,
    b = 0, x = 0 whatever the normals are, and T is the identity to rounding.  With knn = 2 this is the only kind of result
    that can be compared at all: a neighbourhood of two points is a segment, its scatter matrix has two zero eigenvalues, and
    WHICH unit vector across the segment comes back is rounding's choice (Jacobi here, LAPACK in the reference)."""
    rng = np.random.default_rng(seed)
    tgt = corner(rng, nt).astype(f32)
    src = tgt[rng.permutation(nt)[:ns]].copy()
    return src, tgt, np.eye(4, dtype=f32), params(normals_knn=knn)


def knn_jobs():
    s, t, g = pair(1310, 300, 500)
    return {"knn2": subset_job(2), "knn10": (s, t, g, params(normals_knn=10)), "knn16": (s, t, g, params(normals_knn=16))}


def singular_jobs():
    """name -> job whose normal equations have rank < 6: status 5, T = the guess, no iteration counted.  The clouds are
    exact (dyadic, axis-aligned), so that the rank is lost to the bit and not to noise."""
    rng = np.random.default_rng(1400)
    src = corner(rng, 120).astype(f32)
    grid = rng.integers(-384, 385, (300, 3)) / 128.0                      # multiples of 2^-7 within +-3
    flat = grid * np.array([1, 1, 0])                                     # z = 0: every normal is +-z
    wall = grid * np.array([0, 1, 0.5]) + np.array([1.5, 0, 0])           # one wall, x = 1.5
    line = grid * np.array([1, 0, 0]) + np.array([0, 0.5, -0.25])         # collinear along x
    eye = np.eye(4, dtype=f32)
    return {
        "z0_target": (src, flat.astype(f32), eye, params()),
        "one_wall": (src, wall.astype(f32), eye, params()),
        "collinear": (src, line.astype(f32), eye, params()),
        "nt1": (src, np.array([[0.5, -0.25, 0.125]], f32), eye, params()),
        "nt2": (src, np.array([[0.5, -0.25, 0.125], [-1.0, -0.25, 0.125]], f32), eye, params()),
    }


def status_jobs():
    """name -> job, each with the status or the stop it is built for"""
    src, tgt, g = pair(1500, 300, 400)
    far = (src * np.array([1, 1, 0.3], f32) + np.array([0, 0, 3.0], f32)).astype(f32)   # z in 2.7 .. 3.3: 1.5 m above the top
    eye = np.eye(4, dtype=f32)
    nan_guess = g.copy()
    nan_guess[1, 3] = np.nan
    aligned = np.asarray(C3.TRUTH, f32)
    return {
        "no_finite_distance": (far, tgt, aligned, params(matcher_max_dist=1.0)),                         # status 1
        "max_dist_drops_all": (far, tgt, aligned, params(max_dist_filter=0.3)),                          # status 2
        "nan_in_guess": (src, tgt, nan_guess, params()),                                                 # status 1
        "counter_below_smooth": (src, tgt, g, params(max_iter=2)),
        "counter_above_smooth": (src, tgt, g, params(max_iter=6, min_diff_rot=1e-9, min_diff_trans=1e-9)),
        "diff_at_smooth": (src, tgt, aligned, params()),
        "diff_above_smooth": (src, tgt, C3.rigid((0.2, 0.7, -0.4), 0.25, (0.5, 0.4, -0.45)) @ C3.TRUTH,
                              params(min_diff_rot=0.002, min_diff_trans=0.02)),
    }


def sliding_job():
    """Two walls (x = -1.5 and y = -1.5) and a floor patch; the source is a noise-free subset of the target and the guess
    shifts it 0.5 m along the wall y = -1.5.  Point-to-point pays for every source point that slides along its own wall;
    point-to-plane does not.  -> (source, target, guess, point-to-plane params, point-to-point params)"""
    rng = np.random.default_rng(1600)
    n = 600
    w = rng.integers(0, 5, n)
    w = np.where(w < 2, 0, np.where(w < 4, 1, 2))                          # 2 : 2 : 1 over the walls and the patch
    u = rng.uniform(0, 1, (n, 3)) * np.array([3.0, 3.0, 2.0])
    u[w == 2] *= np.array([1.0 / 3, 1.0 / 3, 1.0])                         # the floor patch: 1 x 1 m in the corner
    u[np.arange(n), w] = 0.0
    tgt = (u - np.array([1.5, 1.5, 1.0])).astype(f32)
    src = tgt[rng.permutation(n)[:250]].copy()
    guess = np.eye(4, dtype=f32)
    guess[0, 3] = 0.5
    kw = dict(min_diff_rot=1e-4, min_diff_trans=1e-4, max_iter=60)
    return src, tgt, guess, params(**kw), params(minimizer=0, **kw)


def mixed_launch():
    """-> (sources, targets, [(source index, target index, guess)], params): jobs that share targets and sources, targets
    on either side of the resident tile, a status-5 job (a z = 0 target) between succeeding ones"""
    p = params()
    s0, t0, g0 = pair(1700, 700, 900)
    s1, t1, g1 = pair(1701, 1, TILE + 3)
    s2, t2, g2 = pair(1702, 1200, 300)
    flat = singular_jobs()["z0_target"][1]
    srcs, tgts = [s0, s1, s2], [t0, t1, t2, flat]
    jobs = [(0, 0, g0), (1, 1, g1), (0, 3, g0), (2, 2, g2), (0, 0, g2), (2, 0, g0), (0, 2, g0), (1, 1, g0)]
    return srcs, tgts, jobs, p


def batch_pair():
    return pair(1700, 700, 900)


def batch_guesses(n=30):
    return C3.batch_guesses(n, seed=1800)


# ---- clouds whose normals are compared ----
def normals_cloud(n, seed=None):
    """n noisy points of the box corner (n < 8: a tetrahedron's worth of generic points)"""
    rng = np.random.default_rng(2000 + n if seed is None else seed)
    return corner(rng, n, noise=0.01).astype(f32)


def lattice_tie_cloud():
    """NTILE + 64 points.  Two constellations on a lattice of step 1/8: a centre c, two neighbours at c +- (s, 0, 0), and two
    candidates for the fourth place of c's neighbourhood (knn = 4) at exactly the same distance, a = c + (0, 2 s, 0) and
    b = c + (0, 0, 2 s): the lower index decides between a normal along z and one along y.  In the first constellation a and b
    sit at indices NTILE - 1 and NTILE (either side of the tile edge), in the second at 300 and 200 (inside a tile).
    -> (cloud, knn, [(centre index, chosen index, refused index)])"""
    rng = np.random.default_rng(2100)
    n, s = NTILE + 64, 0.125
    cloud = (rng.integers(-384, 129, (n, 3)) / 128.0)                      # generic points in [-3, 1]^3
    spots = [(np.array([3.0, 3.0, 3.0]), (10, 11, 12, NTILE - 1, NTILE)), (np.array([3.0, -3.0, 3.0]), (20, 21, 22, 300, 200))]
    ties = []
    for c, (ic, i1, i2, ia, ib) in spots:
        cloud[ic], cloud[i1], cloud[i2] = c, c + [s, 0, 0], c - [s, 0, 0]
        cloud[ia], cloud[ib] = c + [0, 2 * s, 0], c + [0, 0, 2 * s]
        ties.append((ic, min(ia, ib), max(ia, ib)))
    return cloud.astype(f32), 4, ties


def degenerate_cloud():
    """200 generic points, 12 coincident ones and a run of 20 collinear ones (along ``direction``, 1/16 apart), both far from
    the rest -> (cloud, knn, indices of the coincident points, indices of the collinear points, direction)"""
    rng = np.random.default_rng(2200)
    gen = corner(rng, 200, noise=0.01)
    same = np.tile([3.0, 3.0, -3.0], (12, 1))
    d = np.array([2.0, -1.0, 2.0]) / 3.0
    run = np.array([-3.0, 3.0, 1.0]) + np.arange(20)[:, None] / 16.0 * d[None, :]
    cloud = np.concatenate([gen, same, run]).astype(f32)
    return cloud, 5, np.arange(200, 212), np.arange(212, 232), d


def nonfinite_cloud():
    """600 corner points, five of them NaN or infinite in some coordinate -> (cloud, knn, their indices)"""
    cloud = normals_cloud(600, seed=2300)
    bad = np.array([7, 100, 255, 256, 599])
    cloud[7, 0] = np.nan
    cloud[100] = np.nan
    cloud[255, 2] = np.inf
    cloud[256, 1] = -np.inf
    cloud[599, 0] = np.nan
    return cloud, 10, bad


NORMALS_SIZES = (1, 2, 3, LANES - 1, LANES, LANES + 1, NTILE - 1, NTILE, NTILE + 1, 2 * NTILE + 1)
NORMALS_KNN = (2, 10, 16)


@functools.lru_cache(maxsize=None)
def normals_ref(n, knn):
    """(normals, gaps) of normals_cloud(n) by the reference, computed once per process"""
    return R.normals(normals_cloud(n), knn, with_gap=True)


# ---- every ICP job the GPU tests run, by name ----
def all_jobs():
    jobs = {}
    for j in source_count_jobs():
        jobs["ns%d" % len(j[0])] = j
    for j in target_count_jobs():
        jobs["nt%d" % len(j[1])] = j
    jobs.update(knn_jobs())
    jobs["subset"] = subset_job(10, seed=1320)
    jobs.update(singular_jobs())
    jobs.update(status_jobs())
    s, t, g, pp, p0 = sliding_job()
    jobs["sliding"] = (s, t, g, pp)
    srcs, tgts, mj, p = mixed_launch()
    for k, (a, b, g) in enumerate(mj):
        jobs["mixed%d" % k] = (srcs[a], tgts[b], g, p)
    s, t, _ = batch_pair()
    for k, gk in enumerate(batch_guesses()):
        jobs["batch%d" % k] = (s, t, gk, params())
    return jobs


@functools.lru_cache(maxsize=None)
def _jobs():
    return all_jobs()


@functools.lru_cache(maxsize=None)
def _normals(key, knn):
    t = _TARGETS[key]
    return R.normals(t, knn, centre=True)


_TARGETS = {}


def target_normals(tgt, knn):
    """the reference normals of a (centred) target, computed once per distinct target and knn"""
    key = (tgt.shape, tgt.tobytes())
    _TARGETS.setdefault(key, tgt)
    return _normals(key, knn)


@functools.lru_cache(maxsize=None)
def ref(name):
    """(status, T, iterations) of the named job by icp3_plane_ref, computed once per process"""
    s, t, g, p = _jobs()[name]
    return R.icp(s, t, g, p, normals_of=target_normals(t, p.normals_knn))


def job(name):
    return _jobs()[name]
