"""Constructed inputs of the 3-D ICP chain tests (tests/test_icp3_chain_host.py on the reference alone,
tests/test_gpu_icp3_chain.py against the device).  Test infrastructure only.

The lattice case makes the matcher's float distances exact, so that pairs sit exactly on a filter's threshold and one ulp
either side of it: the target is the symmetric lattice {-16, -8, 0, 8, 16}^3 (its mean is exactly zero, so the frame's
subtractions change nothing), the guess is the identity, ``max_iter = 1``, and every source point is a lattice point plus a
short dyadic offset.  The nine boundary points belong to the lattice point at the origin, three per axis:
    offset 1.5                  d2 = 2.25 exactly
    offset 1.5 and 2^-11 across d2 = 2.25 + 2^-22, one ulp above (the binade [2, 4) has ulp 2^-22)
    offset 1.5 - 2^-23          d2 = fl(2.25 - 3 2^-23 + 2^-46) = 2.25 - 2^-22, one ulp below
The rest: 40 points at offset 0.5 (d2 0.25), 21 at offset 1 (d2 1), 10 at offset 2 (d2 4), and 44 points 100 m away that
the matcher (maxDist 10) leaves unmatched.  So of the 80 finite d2 the median (rank 40) is exactly 1, while the rank-62 value
among all 124 lies in the boundary group."""
import numpy as np

from sonar_slam_amd import _lib as L
from sonar_slam_amd import icp_config

import icp3_cases

f32 = np.float32
T2 = f32(2.25)                       # the threshold on d2: 1.5^2, and 2.25 x the median 1
ULP = f32(2.0 ** -22)


def lattice_target():
    g = np.array([-16.0, -8.0, 0.0, 8.0, 16.0], f32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(f32)


def lattice_source():
    """-> (source N x 3 float32, group int [N]): group 0 on the threshold, 1 one ulp above, 2 one ulp below, 3 d2 0.25,
    4 d2 1, 5 d2 4, 6 unmatched"""
    rng = np.random.default_rng(77)
    tgt = lattice_target()
    pts, grp = [], []
    below = np.nextafter(f32(1.5), f32(0))
    for a in range(3):
        b = (a + 1) % 3
        for g, (along, across) in enumerate(((f32(1.5), f32(0)), (f32(1.5), f32(2.0 ** -11)), (below, f32(0)))):
            p = np.zeros(3, f32)
            p[a], p[b] = along, across
            pts.append(p)
            grp.append(g)
    others = [i for i in range(len(tgt)) if np.any(tgt[i] != 0)]
    for g, off, count in ((3, 0.5, 40), (4, 1.0, 21), (5, 2.0, 10)):
        for _ in range(count):
            p = tgt[others[rng.integers(len(others))]].copy()
            p[rng.integers(3)] += f32(off) * f32(rng.choice((-1.0, 1.0)))
            pts.append(p)
            grp.append(g)
    for _ in range(44):
        pts.append((f32(100.0) + rng.integers(0, 50, 3)).astype(f32))
        grp.append(6)
    order = rng.permutation(len(pts))
    return np.stack(pts).astype(f32)[order], np.asarray(grp)[order]


def lattice_params(**kw):
    """maxDist 10, no MaxDist / Trimmed filter, one iteration"""
    over = dict(matcher_max_dist=10.0, use_max_dist_filter=0, use_trimmed_filter=0, max_iter=1, use_diff_checker=0)
    over.update(kw)
    return icp_config.shipped_params(**over)


def outliers(**kw):
    return L.IcpOutliers(**kw)


MIN_DIST_ON = dict(use_min_dist=1, min_dist=1.5)            # fl(1.5 1.5) = 2.25: the on-threshold pairs are kept (>=)
MEDIAN_ON = dict(use_median=1, median_factor=2.25)          # fl(2.25 x 1) = 2.25: the on-threshold pairs are kept (<=)


def chain3(params, reading=(), reference=(), **ox):
    return icp_config.IcpChain(params, reading, reference, L.IcpOutliers(**ox) if ox else None, dims=3)


def pair(seed, ns, nt, **kw):
    """a random 3-D scan pair (icp3_cases.pair): a 6 x 6 x 4 m box, the guess a few centimetres and degrees off"""
    return icp3_cases.pair(seed, ns, nt, **kw)


def far_source(n):
    """n points that no target of ``pair`` is within the matcher's 10 m of"""
    rng = np.random.default_rng(5)
    return (rng.uniform(-1, 1, (n, 3)) + np.array([300.0, 0.0, 0.0])).astype(f32)
