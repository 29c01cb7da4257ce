"""numpy restatement of the data-point filters of a 3-D ICP chain (MaxDist, MinDist, BoundingBox on N x 3 clouds: the rules
of include/sonarfe.h at ``sfe_icp3_filter_clouds_dev``), ``dpf_ref`` with one more coordinate: float32 like the device,
every product and sum rounded to float, a correctly rounded square root, strict comparisons.  The octree stage is
``pcl3_ref.downsample``.  Test infrastructure only; the product never imports it."""
import numpy as np

from sonar_slam_amd import _lib as L

import pcl3_ref

f32 = np.float32


def norm(x, y, z):
    """sqrtf(fl(fl(fl(x x) + fl(y y)) + fl(z z)))"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt(f32(f32(f32(x * x) + f32(y * y)) + f32(z * z)), dtype=f32)


def keep_mask(pts, st):
    """bool [N]: the points of pts (N x 3 float32) that the predicate stage st (IcpDpf) keeps"""
    pts = np.ascontiguousarray(pts, f32).reshape(-1, 3)
    x, y, z = (np.ascontiguousarray(pts[:, a]) for a in range(3))
    f = [f32(v) for v in st.f]
    with np.errstate(invalid="ignore", over="ignore"):
        if st.kind == L.DPF_BOUNDING_BOX:
            inside = (f[0] < x) & (x < f[1]) & (f[2] < y) & (y < f[3]) & (f[4] < z) & (z < f[5])
            return inside != bool(st.remove_inside)
        if st.kind not in (L.DPF_MAX_DIST, L.DPF_MIN_DIST):
            raise ValueError("not a predicate stage: %r" % st)
        if st.dim < 0:
            v, thr = norm(x, y, z), np.abs(f[0])
        else:
            v, thr = (x, y, z)[st.dim], f[0]
            if st.kind == L.DPF_MIN_DIST:
                v, thr = np.abs(v), np.abs(f[0])
        return v < thr if st.kind == L.DPF_MAX_DIST else v > thr


def apply(pts, stages, downsample=None):
    """the stages in order on one cloud (N x 3 float32); kept points keep their order.  Octree stages go through
    ``downsample(points, maxSizeByNode) -> points`` (default: ``pcl3_ref.downsample``'s medoids)"""
    if downsample is None:
        downsample = lambda p, size: pcl3_ref.downsample(p, size)[0]        # noqa: E731
    out = np.ascontiguousarray(pts, f32).reshape(-1, 3)
    for st in stages:
        if not isinstance(st, L.IcpDpf):
            continue                       # SurfaceNormal keeps every point
        if st.kind == L.DPF_OCTREE_GRID:
            if len(out):
                out = np.ascontiguousarray(downsample(out, float(st.f[0])), f32).reshape(-1, 3)
        else:
            out = out[keep_mask(out, st)]
    return out


def stage(kind, dim=-1, remove_inside=0, f=()):
    st = L.IcpDpf()
    st.kind, st.dim, st.remove_inside = kind, dim, remove_inside
    for i, v in enumerate(f):
        st.f[i] = v
    return st


def max_dist(v, dim=-1):
    return stage(L.DPF_MAX_DIST, dim, f=(v,))


def min_dist(v, dim=-1):
    return stage(L.DPF_MIN_DIST, dim, f=(v,))


def box(lo, hi, remove_inside=0):
    return stage(L.DPF_BOUNDING_BOX, -1, remove_inside, (lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]))


def octree(size):
    return stage(L.DPF_OCTREE_GRID, f=(size,))
