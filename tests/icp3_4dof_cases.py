"""The inputs of tests/test_gpu_icp3_4dof.py (``sfe_icp_params.minimizer == 3``: point-to-plane solved for yaw and
translation only), built here so that tests/test_icp3_4dof_host.py can hold every one of them to its conditions on the CPU --
the reference with its sums reversed, and with its normals moved by an ulp, lands on itself; the cases built for a status,
a stop or a rank have it -- and so that both files share one reference result per job (``ref``, cached).  A job is (source
N x 3, target M x 3, guess 4 x 4, IcpParams with minimizer 3).  The scenes are the three-wall corner of
``icp3_plane_cases``; the motions are what the minimiser can represent, a rotation about z and a translation, except where
a case says otherwise.  Coordinates stay within +-4 m.  Test infrastructure only."""
import functools

import numpy as np

from sonar_slam_amd import icp_config

import icp3_4dof_ref as R4
import icp3_cases as C3
import icp3_plane_cases as CP

f32 = np.float32
THREADS = C3.THREADS    # queries per pass of the job kernel's workgroup
TILE = C3.TILE          # target points resident in the job kernel's LDS

Z = (0.0, 0.0, 1.0)
TRUTH = C3.rigid(Z, 0.06, (0.15, -0.1, 0.08))                       # yaw and translation: what a 4-DoF step can reach
GUESS = C3.rigid(Z, 0.03, (0.08, 0.05, -0.06)) @ TRUTH

SOURCE_COUNTS = (1, 2, 3, 255, 256, 257, THREADS - 1, THREADS, THREADS + 1, 2 * THREADS + 1)
TARGET_COUNTS = (3, TILE - 1, TILE, TILE + 1)
KNN = (2, 10, 16)


def params(**kw):
    kw.setdefault("minimizer", 3)
    return icp_config.shipped_params(**kw)


def pair(seed, ns, nt, truth=TRUTH, guess=GUESS, **kw):
    """``icp3_plane_cases.pair`` (the three-wall corner) under a yaw-and-translation motion"""
    return CP.pair(seed, ns, nt, truth=truth, guess=guess, **kw)


def source_count_jobs():
    return {"ns%d" % ns: pair(4100 + ns, ns, 300) + (params(),) for ns in SOURCE_COUNTS}


def target_count_jobs():
    return {"nt%d" % nt: pair(4200 + k, 200, nt) + (params(),) for k, nt in enumerate(TARGET_COUNTS)}


def knn_jobs():
    """knn = 2 on the subset under the identity (``icp3_plane_cases.subset_job`` says why nothing else can be compared
    there: the normal of a two-point neighbourhood is rounding's choice); 10 and 16 on one pair"""
    s, t, g = pair(4310, 300, 500)
    s2, t2, g2, _ = CP.subset_job(2, seed=4300)
    return {"knn2": (s2, t2, g2, params(normals_knn=2)), "knn10": (s, t, g, params(normals_knn=10)),
            "knn16": (s, t, g, params(normals_knn=16))}


def roll_job():
    """The corner seen from a frame that is rolled by 2 degrees about x on top of a yaw and a shift; the guess rotates about
    z only.  The 4-DoF minimiser cannot put the roll into T, the 6-DoF one does.  -> (source, target, guess, 4-DoF params,
    6-DoF params)"""
    truth = C3.rigid((1.0, 0.0, 0.0), np.deg2rad(2.0), (0.0, 0.0, 0.0)) @ TRUTH
    s, t, g = pair(4400, 500, 700, truth=truth, guess=GUESS)
    return s, t, g, params(), params(minimizer=2)


def _grid(rng, n):
    return rng.integers(-384, 385, (n, 3)) / 128.0                       # multiples of 2^-7 within +-3


UPRIGHT_KNN = 4


def upright_walls():
    """Four upright walls, x = +-1.5 and y = +-3, whose normals all have n_z = 0 TO THE BIT in the reference (LAPACK) and on
    the device (Jacobi) alike: each wall is made of squares of four points, 0.25 m wide and 1 m apart, so that with
    ``normals_knn = 4`` every neighbourhood is one square; the cloud is its own mirror image through the origin, so its mean
    is exactly zero and the centring changes nothing; every coordinate is dyadic.  The scatter matrix of a square is then
    exactly diagonal with a zero on the wall's axis, and both eigen-solvers leave a diagonal matrix alone.  (A wall of
    random points would do for x = const, whose zero row LAPACK's tridiagonalisation never touches, but not for y = const:
    there eigh returns n_z = 1e-16, a rank that rounding decides.)"""
    h = 0.125
    sq = np.array([[-h, -h], [h, -h], [-h, h], [h, h]])
    walls = []
    for u in (-2.0, -1.0, 0.0, 1.0, 2.0):
        for w in (-1.0, 0.0, 1.0):
            walls.append(np.stack([np.full(4, 1.5), u + sq[:, 0], w + sq[:, 1]], 1))           # x = 1.5
    for u in (-1.0, 0.0, 1.0):
        for w in (-1.0, 0.0, 1.0):
            walls.append(np.stack([u + sq[:, 0], np.full(4, 3.0), w + sq[:, 1]], 1))           # y = 3
    half = np.concatenate(walls)
    cloud = np.concatenate([half, -half])
    return cloud[np.random.default_rng(4510).permutation(len(cloud))]


def rank_jobs():
    """name -> job whose 4 x 4 system has rank < 4 (status 5, T = the guess, no iteration counted) or no kept pair (status
    2).  The targets are exact (dyadic, axis-aligned), so that the rank is lost to the bit and not to noise:
      z0_target        every normal is +-z: c = 0 and n_x = n_y = 0, only t_z is seen (rank 1)
      one_wall         x = 1.5, every normal +-x: F = (-p_y n_x, n_x, 0, 0) (rank 2)
      upright_walls    ``upright_walls``, every normal +-x or +-y: n_z = 0, t_z is free (rank 3)
      one_source_point one pair (rank 1)
      empty_keep_set   MaxDist drops every pair"""
    rng = np.random.default_rng(4500)
    src = CP.corner(rng, 120).astype(f32)
    g = _grid(rng, 300)
    flat = g * np.array([1, 1, 0])
    wall = g * np.array([0, 1, 0.5]) + np.array([1.5, 0, 0])
    upright = upright_walls()
    eye = np.eye(4, dtype=f32)
    s1, t1, g1 = pair(4501, 1, 300)
    s2, t2, g2 = pair(4502, 300, 400)
    far = (s2 * np.array([1, 1, 0.3], f32) + np.array([0, 0, 3.0], f32)).astype(f32)     # 1.5 m above the corner's top
    return {
        "z0_target": (src, flat.astype(f32), eye, params()),
        "one_wall": (src, wall.astype(f32), eye, params()),
        "upright_walls": (src, upright.astype(f32), eye, params(normals_knn=UPRIGHT_KNN)),
        "one_source_point": (s1, t1, g1, params()),
        "empty_keep_set": (far, t2, np.asarray(TRUTH, f32), params(max_dist_filter=0.3)),
    }


EXACT_SINGULAR = ("z0_target", "one_wall", "upright_walls")     # status 5 by exact zeros: every normal is +-an axis
RANK_STATUS = {"z0_target": 5, "one_wall": 5, "upright_walls": 5, "one_source_point": 5, "empty_keep_set": 2}


def status_jobs():
    """name -> job, each with the status or the stop it is built for (the shapes of ``icp3_plane_cases.status_jobs``)"""
    src, tgt, g = pair(4600, 300, 400)
    far = (src * np.array([1, 1, 0.3], f32) + np.array([0, 0, 3.0], f32)).astype(f32)
    nan_guess = g.copy()
    nan_guess[1, 3] = np.nan
    aligned = np.asarray(TRUTH, f32)
    return {
        "no_finite_distance": (far, tgt, aligned, params(matcher_max_dist=1.0)),                         # status 1
        "max_dist_drops_all": (far, tgt, aligned, params(max_dist_filter=0.3)),                          # status 2
        "nan_in_guess": (src, tgt, nan_guess, params()),                                                 # status 1
        "counter_below_smooth": (src, tgt, g, params(max_iter=2)),
        "counter_above_smooth": (src, tgt, g, params(max_iter=6, min_diff_rot=1e-9, min_diff_trans=1e-9)),
        "diff_at_smooth": (src, tgt, aligned, params()),
        "diff_above_smooth": (src, tgt, C3.rigid(Z, 0.25, (0.5, 0.4, -0.45)) @ TRUTH,
                              params(min_diff_rot=0.002, min_diff_trans=0.02)),
    }


def mixed_launch():
    """-> (sources, targets, [(source index, target index, guess)], params): jobs of different sizes that share targets and
    sources, targets on either side of the resident tile, status-5 jobs (a z = 0 target, a single source point) beside
    succeeding ones"""
    p = params()
    s0, t0, g0 = pair(4700, 700, 900)
    s1, t1, g1 = pair(4701, 1, TILE + 3)
    s2, t2, g2 = pair(4702, 1200, 300)
    flat = rank_jobs()["z0_target"][1]
    srcs, tgts = [s0, s1, s2], [t0, t1, t2, flat]
    jobs = [(0, 0, g0), (1, 1, g1), (0, 3, g0), (2, 2, g2), (0, 0, g2), (2, 0, g0), (0, 2, g0), (2, 1, g0)]
    return srcs, tgts, jobs, p


MIXED_STATUS = [0, 5, 5, 0, 0, 0, 0, 0]


def batch_pair():
    return pair(4700, 700, 900)


def batch_guesses(n=30):
    """GUESS with small random yaw-and-translation motions in front"""
    rng = np.random.default_rng(4800)
    return [np.asarray(C3.rigid(Z, rng.uniform(-0.06, 0.06), rng.uniform(-0.15, 0.15, 3)) @ GUESS, f32) for _ in range(n)]


# ---- every ICP job the GPU tests run, by name ----
def all_jobs():
    jobs = {}
    jobs.update(source_count_jobs())
    jobs.update(target_count_jobs())
    jobs.update(knn_jobs())
    jobs.update(rank_jobs())
    jobs.update(status_jobs())
    s, t, g, p4, p6 = roll_job()
    jobs["roll"] = (s, t, g, p4)
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


def target_normals(tgt, knn):
    """the reference normals of a (centred) target, computed once per distinct target and knn"""
    return CP.target_normals(tgt, knn)


@functools.lru_cache(maxsize=None)
def ref(name):
    """(status, T, iterations) of the named job by icp3_4dof_ref, computed once per process"""
    s, t, g, p = _jobs()[name]
    return R4.icp(s, t, g, p, normals_of=target_normals(t, p.normals_knn))


def job(name):
    return _jobs()[name]
