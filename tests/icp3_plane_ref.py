"""numpy restatement of the 3-D point-to-plane chain of ``sfe_icp3_compute_jobs`` (``sfe_icp_params.minimizer == 2``;
include/sonarfe.h states the rules at ``sfe_normals3`` and ``sfe_icp3_compute_jobs``): the surface normals of a cloud by
``np.linalg.eigh`` and the ICP loop with ``np.linalg.solve`` behind the Cholesky pivot test.  Frame, matcher, outlier filters
and checkers are ``icp3_ref``'s, whose ``mat4``, ``affine``, ``nn``, ``quat`` and ``quat_dist`` this module uses.  Test
infrastructure only; the product never imports it.

Switches, in ``icp3_ref``'s style: ``reverse_sums`` takes the fp64 sums in reversed pair order; ``tie_high`` gives equal
neighbour distances to the HIGHEST index (the wrong rule, to show that an input depends on the right one);
``jitter_normals`` (a seed) moves every normal by one float ulp in a random component and renormalises it."""
import numpy as np

import icp3_ref
from icp3_ref import MAX_HIST, f32

PIVOT_RTOL = 1e-10      # ICP_PIVOT_RTOL
KMAX = 16               # ICP_KMAX


def knn(t, k, tie_high=False):
    """t: three float32 columns.  -> ids [n x k] int64: the k nearest points of every point, itself included, in
    lexicographic (d2, index) order, d2 = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)); -1 from the first neighbour on whose
    d2 is not below +inf (NaN included)"""
    n = len(t[0])
    k = min(k, n)
    ids = np.empty((n, k), np.int64)
    idx = np.arange(n, dtype=np.uint64)
    low = (np.uint64(n - 1) - idx) if tie_high else idx
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, n, 256):
            dx = t[0][a:a + 256, None] - t[0][None, :]
            dy = t[1][a:a + 256, None] - t[1][None, :]
            dz = t[2][a:a + 256, None] - t[2][None, :]
            d = (dx * dx + dy * dy) + dz * dz
            d = np.where(np.isnan(d), f32(np.inf), d) + f32(0.0)          # (-0 -> +0: bit order == value order)
            key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | low[None, :]
            part = np.sort(np.partition(key, k - 1, axis=1)[:, :k], axis=1)
            j = (part & np.uint64(0xFFFFFFFF)).astype(np.int64)
            if tie_high:
                j = n - 1 - j
            j[(part >> np.uint64(32)) >= np.uint64(0x7F800000)] = -1
            ids[a:a + 256] = j
    return ids


def scatter(t, ids):
    """-> (C [n x 3 x 3], count [n]): the fp64 scatter matrices sum (u - m)(u - m)^T of the neighbourhoods, neighbours in
    order, m their mean"""
    n, k = ids.shape
    P = np.stack([np.asarray(c, f32).astype(np.float64) for c in t], 1)
    ok = ids >= 0
    cnt = ok.sum(1)
    U = np.where(ok[:, :, None], P[np.maximum(ids, 0)], 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.cumsum(U, axis=1)[:, -1, :] / cnt[:, None]
        D = np.where(ok[:, :, None], U - m[:, None, :], 0.0)
    C = np.cumsum(D[:, :, :, None] * D[:, :, None, :], axis=1)[:, -1]
    C[cnt == 0] = 0.0
    return C, cnt


def normals(pts, k, tie_high=False, centre=False, with_gap=False):
    """The surface normals of an N x 3 float32 cloud -> float32 [N x 3] (``with_gap``: also the relative eigen-gap
    (l2 - l1) / l3 of every neighbourhood, 0 where l3 == 0).  ``centre``: on the cloud centred the way the ICP centres its
    target.  The sign is eigh's; C = 0 gives (1, 0, 0)."""
    pts = np.ascontiguousarray(pts, f32).reshape(-1, 3)
    t = centred(pts)[1] if centre else tuple(pts[:, a].copy() for a in range(3))
    C, _ = scatter(t, knn(t, min(k, KMAX), tie_high))
    bad = ~np.isfinite(C).all(axis=(1, 2))
    C[bad] = 0.0
    w, v = np.linalg.eigh(C)
    nv = v[:, :, 0]
    nv = nv / np.linalg.norm(nv, axis=1)[:, None]
    nv[(C == 0).all(axis=(1, 2))] = (1.0, 0.0, 0.0)
    if with_gap:
        with np.errstate(invalid="ignore", divide="ignore"):
            gap = np.where(w[:, 2] > 0, (w[:, 1] - w[:, 0]) / w[:, 2], 0.0)
        return nv.astype(f32), gap
    return nv.astype(f32)


def centred(tgt):
    """-> (mean float32 [3], the three float32 columns of the target centred on it), as the kernel centres it"""
    nt = len(tgt)
    with np.errstate(invalid="ignore", over="ignore"):
        mean = np.array([f32(np.cumsum(tgt[:, a].astype(np.float64))[-1] / nt) for a in range(3)], f32)
        return mean, tuple(tgt[:, a] - mean[a] for a in range(3))


def jitter(nv, seed):
    """every normal moved by one float ulp in a seeded random component, renormalised"""
    rng = np.random.default_rng(seed)
    out = nv.copy()
    comp = rng.integers(0, 3, len(nv))
    up = rng.random(len(nv)) < 0.5
    rows = np.arange(len(nv))
    out[rows, comp] = np.nextafter(out[rows, comp], np.where(up, f32(np.inf), f32(-np.inf)).astype(f32))
    o = out.astype(np.float64)
    return (o / np.linalg.norm(o, axis=1)[:, None]).astype(f32)


def rodrigues(r):
    """the rotation by |r| about r / |r|, fp64; the identity for |r| == 0"""
    th = np.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
    if th == 0.0:
        return np.eye(3)
    k = r / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def singular(A):
    """the Cholesky pivot rule of the 2-D minimiser on a symmetric 6 x 6 matrix: A00 > 0 and every later pivot above
    PIVOT_RTOL times its diagonal entry, else singular (NaN included)"""
    n = len(A)
    L = np.zeros((n, n))
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(n):
            piv = A[j, j] - np.dot(L[j, :j], L[j, :j])
            if not (piv > 0 if j == 0 else piv > PIVOT_RTOL * A[j, j]):
                return True
            L[j, j] = np.sqrt(piv)
            for i in range(j + 1, n):
                L[i, j] = (A[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    return False


def system(P, Q, N, reverse_sums=False):
    """kept pairs (fp64 [m x 3] each: moved reading points, centred target points, their normals) -> (A 6 x 6, b 6)"""
    c = np.stack([P[:, 1] * N[:, 2] - P[:, 2] * N[:, 1], P[:, 2] * N[:, 0] - P[:, 0] * N[:, 2],
                  P[:, 0] * N[:, 1] - P[:, 1] * N[:, 0]], 1)
    F = np.concatenate([c, N], 1)
    D = P - Q
    e = (N[:, 0] * D[:, 0] + N[:, 1] * D[:, 1]) + N[:, 2] * D[:, 2]
    if reverse_sums:
        F, e = F[::-1], e[::-1]
    A = np.cumsum(F[:, :, None] * F[:, None, :], axis=0)[-1]
    b = -np.cumsum(F * e[:, None], axis=0)[-1]
    return A, b


def icp(src, tgt, guess, p, reverse_sums=False, tie_high=False, jitter_normals=None, trace=None, normals_of=None):
    """-> (status, T 4 x 4 float32, iterations) of one job.  p: IcpParams with minimizer 2.  ``trace``: a list that receives
    (ids, d2, keep) of every iteration; ``normals_of``: the target's normals, if the caller has them already (they depend on
    the target and ``normals_knn`` only)."""
    assert p.minimizer == 2
    src = np.ascontiguousarray(src, f32).reshape(-1, 3)
    tgt = np.ascontiguousarray(tgt, f32).reshape(-1, 3)
    guess = np.asarray(guess, f32).reshape(4, 4)
    mean, t = centred(tgt)
    nv = normals_of if normals_of is not None else normals(tgt, p.normals_knn, tie_high=tie_high, centre=True)
    if jitter_normals is not None:
        nv = jitter(nv, jitter_normals)
    nv = nv.astype(np.float64)
    T0 = icp3_ref.mat4(icp3_ref.translate(-mean), guess)
    r = icp3_ref.affine(T0, src[:, 0], src[:, 1], src[:, 2])
    r2_match = f32(f32(p.matcher_max_dist) * f32(p.matcher_max_dist))
    r2_filter = f32(f32(p.max_dist_filter) * f32(p.max_dist_filter))
    Ti = np.eye(4, dtype=f32)
    hist = [Ti.copy()]
    status, iters, counter = 0, 0, 0
    while True:
        c = icp3_ref.affine(Ti, *r)
        ids, d2 = icp3_ref.nn(c, t, r2_match)
        keep = ids >= 0
        fin = d2[keep]
        if p.use_max_dist_filter:
            keep = keep & (d2 <= r2_filter)
        if p.use_trimmed_filter:
            if len(fin) == 0:
                status = 1
                break
            k = len(fin) - 1 if p.trim_ratio >= 1.0 else int(f32(len(fin)) * f32(p.trim_ratio))
            keep = keep & (d2 <= icp3_ref._kth(fin, k))
        if trace is not None:
            trace.append((ids.copy(), d2.copy(), keep.copy()))
        if not keep.any():
            status = 2
            break
        P = np.stack([v[keep].astype(np.float64) for v in c], 1)
        q = ids[keep]
        Q = np.stack([v[q].astype(np.float64) for v in t], 1)
        A, b = system(P, Q, nv[q], reverse_sums)
        if singular(A):
            status = 5
            break
        x = np.linalg.solve(A, b)
        Ts = np.eye(4)
        Ts[:3, :3] = rodrigues(x[:3])
        Ts[:3, 3] = x[3:]
        Ti = icp3_ref.mat4(Ts.astype(f32), Ti)
        iters += 1
        counter += 1
        iterate = True
        if counter >= p.max_iter:
            iterate = False
        elif p.use_diff_checker:
            hist.append(Ti.copy())
            hist = hist[-MAX_HIST:]
            if iters + 1 > p.smooth_len:
                rsum = tsum = 0.0
                for i in range(len(hist) - 1, len(hist) - 1 - p.smooth_len, -1):
                    a, bb = hist[i].astype(np.float64), hist[i - 1].astype(np.float64)
                    rsum += icp3_ref.quat_dist(icp3_ref.quat(a[:3, :3]), icp3_ref.quat(bb[:3, :3]))
                    d = a[:3, 3] - bb[:3, 3]
                    tsum += np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
                rsum /= p.smooth_len
                tsum /= p.smooth_len
                if rsum < f32(p.min_diff_rot) and tsum < f32(p.min_diff_trans):
                    iterate = False
                if np.isnan(rsum):
                    status = 3
                elif np.isnan(tsum):
                    status = 4
        if status != 0 or not iterate:
            break
    if status != 0:
        return status, guess.copy(), iters
    return status, icp3_ref.mat4(icp3_ref.translate(mean), icp3_ref.mat4(Ti, T0)), iters
