"""numpy float32 restatement of the cloud functions of ``pcl`` on N x 3 clouds ("3-D clouds"): the 2-D
rules of oracle/sonar_oracle.c with one more coordinate.  Every product and sum is a separate float32 numpy operation, so
nothing is contracted:

    d2 = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz))

With z = 0 on both sides the third term is +0 and every function gives what the oracle's 2-D function gives on (x, y)
(tests/test_pcl3_host.py), which ties this file to the pinned 2-D behaviour.  Test infrastructure only.
"""
import numpy as np

F = np.float32
MAX_LEVELS = 21     # 3 key bits per level in a 64-bit path key (S3_MAX_LEVELS, sfe_octree3.h)


def _c3(a):
    a = np.ascontiguousarray(a, F)
    assert a.ndim == 2 and a.shape[1] == 3, a.shape
    return a


def dist2(p, q):
    """squared distances of the rows of q [n x 3] from p ([3] or [n x 3]), float32, in the kernels' order"""
    with np.errstate(over="ignore", invalid="ignore"):   # (points 3e19 apart: +inf, as in C)
        d = (p - q).astype(F)
        a, b, c = d[..., 0] * d[..., 0], d[..., 1] * d[..., 1], d[..., 2] * d[..., 2]
        return ((a + b).astype(F) + c).astype(F)


def match_knn(ref, pts, knn, max_dist):
    """-> (ids int32 [knn x N], d2 float32 [knn x N]): ascending (d2, index), -1 / inf beyond the radius.  A reference
    point at d2 = +inf is no neighbour for any max_dist, inf included (the kernels' and oracle.match's d < best from an
    infinite best; recalled to be libnabo's strict heap test too, parity unpinned)."""
    ref, pts = _c3(ref), _c3(pts)
    with np.errstate(over="ignore"):
        r2 = F(max_dist) * F(max_dist)                   # float * float, as sfe_match forms it
    ids = np.full((knn, len(pts)), -1, np.int32)
    d2 = np.full((knn, len(pts)), np.inf, F)
    for i, p in enumerate(pts):
        d = dist2(p, ref)
        order = np.argsort(d, kind="stable")[:knn]       # stable: ties -> the lowest reference index
        ok = (d[order] <= r2) & (d[order] < F(np.inf))   # (NaN: never; +inf: never, even with r2 = inf)
        ids[:len(order), i] = np.where(ok, order, -1)
        d2[:len(order), i] = np.where(ok, d[order], F(np.inf))
    return ids, d2


def match(ref, pts, max_dist):
    return match_knn(ref, pts, 1, max_dist)


def remove_outlier(pts, radius, min_points, return_mask=False):
    pts = _c3(pts)
    r2 = F(float(radius) * float(radius))
    keep = np.array([int((dist2(p, pts) <= r2).sum()) > int(min_points) for p in pts], bool).reshape(len(pts))
    return (pts[keep].copy(), keep) if return_mask else pts[keep].copy()


def knn_density(pts, knn):
    pts = _c3(pts)
    if knn > len(pts):
        raise RuntimeError("Requesting more points than available in cloud")
    ids, _ = match_knn(pts, pts, knn, np.inf)            # incl. self; a point at d2 = +inf is no neighbour: ids -1
    have = ids >= 0
    real = have.sum(axis=0).astype(F)                    # the real neighbours: what the C oracle and the kernels divide by
    s = np.zeros((len(pts), 3), F)
    with np.errstate(all="ignore"):
        for j in range(knn):                             # one chain of additions per coordinate, in neighbour order
            s = np.where(have[j][:, None], (s + pts[ids[j]]).astype(F), s)
        mean = (s / real[:, None]).astype(F)
        rmax = np.zeros(len(pts), F)
        for j in range(knn):                             # fmax: a NaN distance never raises the maximum (r > rmax in C)
            rmax = np.where(have[j], np.fmax(rmax, np.sqrt(dist2(pts[ids[j]], mean)).astype(F)), rmax)
        r = rmax.astype(np.float64)
        volume = ((4. / 3.) * 3.14159265358979323846 * (r * r * r)).astype(F)
        return (real / volume).astype(F)


def max_size_of(resolution):
    """std::to_string(float) and back (pcl.cpp:134)"""
    return F(float("%f" % F(resolution)))


def downsample(pts, resolution, info=None):
    """-> (medoids [m x 3], their input indices int32 [m]) in leaf-visit order.  ``info`` (a dict, optional) receives
    "leaves" (the input indices of every leaf, in visit order), "depth" (the deepest leaf) and "ties" (per leaf: how
    many of its points attain the minimum centroid distance)."""
    pts = _c3(pts)
    max_size = max_size_of(resolution)
    out, leaves, ties, depth_seen = [], [], [], [0]
    if len(pts) == 0:
        return pts.copy(), np.zeros(0, np.int32)

    def node(ids, c, r, depth):
        if len(ids) == 0:
            return
        if float(r) * 2.0 <= float(max_size) or len(ids) <= 1 or depth >= MAX_LEVELS:
            s = np.zeros(3, F)
            for i in ids:                                # float centroid: one chain of additions, input order
                s = (s + pts[i]).astype(F)
            s = (s / F(len(ids))).astype(F)
            d = np.sqrt(dist2(pts[ids], s)).astype(F)
            out.append(int(ids[int(np.argmin(d))]))      # argmin: the first point at the minimum
            leaves.append(ids)
            ties.append(int((d == d.min()).sum()))
            depth_seen[0] = max(depth_seen[0], depth)
            return
        p = pts[ids]
        child = (p[:, 0] > c[0]).astype(int) | ((p[:, 1] > c[1]).astype(int) << 1) | ((p[:, 2] > c[2]).astype(int) << 2)
        hr = F(r * F(0.5))
        for k in range(8):                               # index order, depth first; boolean masks keep the input order
            sign = np.array([hr if k & 1 else -hr, hr if k & 2 else -hr, hr if k & 4 else -hr], F)
            node(ids[child == k], (c + sign).astype(F), hr, depth + 1)

    mn, mx = pts.min(axis=0), pts.max(axis=0)
    ext = (mx - mn).astype(F)
    centre = (mn + (ext * F(0.5)).astype(F)).astype(F)
    node(np.arange(len(pts)), centre, F(ext.max() * F(0.5)), 0)
    if info is not None:
        info.update(leaves=leaves, ties=ties, depth=depth_seen[0])
    idx = np.array(out, np.int32)
    return pts[idx].copy(), idx
