"""numpy restatement of the 4-DoF point-to-plane step of ``sfe_icp3_compute_jobs`` (``sfe_icp_params.minimizer == 3``,
libpointmatcher's ``PointToPlaneErrorMinimizer {force4DOF: 1}``; include/sonarfe.h states the rule under "minimizer 3"): per
kept pair F = (p_x n_y - p_y n_x, n_x, n_y, n_z) and e = n . (p - q) widened to fp64, the sums A = sum F F^T and b = -sum F e,
``np.linalg.solve`` on the 4 x 4 system behind the Cholesky pivot test, the rotation by x[0] about z and the translation
x[1:4].  Everything else -- frame, matcher, normals, outlier filters, checkers, and with ``ox`` the MinDist / MedianDist /
Bound modules of a chain -- is the loop of ``icp3_plane_ref.icp`` / ``icp3_chain_ref.icp``, whose pieces this module
imports.  Test infrastructure only; the product never imports it.

Switches, in ``icp3_plane_ref``'s style: ``reverse_sums`` takes the fp64 sums in reversed pair order; ``jitter_normals`` (a
seed) moves every normal by one float ulp in a random component and renormalises it."""
import numpy as np

import icp3_chain_ref
import icp3_plane_ref
import icp3_ref
from icp3_ref import MAX_HIST, f32, mat4, nn, quat, quat_dist

PIVOT_RTOL = icp3_plane_ref.PIVOT_RTOL


def singular(A):
    """the Cholesky pivot rule on the symmetric 4 x 4 matrix (``icp3_plane_ref.singular`` takes any size)"""
    return icp3_plane_ref.singular(np.asarray(A, np.float64))


def rot_z(gamma):
    """the rotation by gamma about z, fp64: AngleAxis(gamma, UnitZ)"""
    c, s = np.cos(gamma), np.sin(gamma)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def system(P, Q, N, reverse_sums=False):
    """kept pairs (fp64 [m x 3] each: moved reading points, centred target points, their normals) -> (A 4 x 4, b 4)"""
    c = P[:, 0] * N[:, 1] - P[:, 1] * N[:, 0]
    F = np.concatenate([c[:, None], N], 1)
    D = P - Q
    e = (N[:, 0] * D[:, 0] + N[:, 1] * D[:, 1]) + N[:, 2] * D[:, 2]
    if reverse_sums:
        F, e = F[::-1], e[::-1]
    A = np.cumsum(F[:, :, None] * F[:, None, :], axis=0)[-1]
    b = -np.cumsum(F * e[:, None], axis=0)[-1]
    return A, b


def step(A, b):
    """-> (R 3 x 3, t 3) fp64 of a system that does not count as singular"""
    x = np.linalg.solve(A, b)
    return rot_z(x[0]), x[1:4]


def icp(src, tgt, guess, p, ox=None, reverse_sums=False, jitter_normals=None, trace=None, normals_of=None):
    """-> (status, T 4 x 4 float32, iterations) of one job.  p: IcpParams with minimizer 3; ox: IcpOutliers or None (the
    MinDist / MedianDist / Bound modules of a chain).  ``trace``: a list that receives (ids, d2, keep) of every iteration;
    ``normals_of``: the centred target's normals, if the caller has them already."""
    assert p.minimizer == 3
    src = np.ascontiguousarray(src, f32).reshape(-1, 3)
    tgt = np.ascontiguousarray(tgt, f32).reshape(-1, 3)
    guess = np.asarray(guess, f32).reshape(4, 4)
    use_med = bool(ox is not None and ox.use_median)
    use_bound = bool(ox is not None and ox.use_bound)
    mean, t = icp3_plane_ref.centred(tgt)
    nv = normals_of if normals_of is not None else icp3_plane_ref.normals(tgt, p.normals_knn, centre=True)
    if jitter_normals is not None:
        nv = icp3_plane_ref.jitter(nv, jitter_normals)
    nv = nv.astype(np.float64)
    T0 = mat4(icp3_ref.translate(-mean), guess)
    r = icp3_ref.affine(T0, src[:, 0], src[:, 1], src[:, 2])
    r2_match = f32(f32(p.matcher_max_dist) * f32(p.matcher_max_dist))
    r2_filter = f32(f32(p.max_dist_filter) * f32(p.max_dist_filter))
    Ti = np.eye(4, dtype=f32)
    hist = [Ti.copy()]
    status, iters, counter = 0, 0, 0
    while True:
        c = icp3_ref.affine(Ti, *r)
        ids, d2 = nn(c, t, r2_match)
        keep = ids >= 0
        fin = d2[keep]
        if p.use_max_dist_filter:
            keep = keep & (d2 <= r2_filter)
        if (p.use_trimmed_filter or use_med) and len(fin) == 0:
            status = 1                                 # "no outlier to filter"
            break
        if p.use_trimmed_filter:
            k = len(fin) - 1 if p.trim_ratio >= 1.0 else int(f32(len(fin)) * f32(p.trim_ratio))
            keep = keep & (d2 <= icp3_ref._kth(fin, k))
        med_limit = f32(np.inf)
        if use_med:
            med_limit = f32(f32(ox.median_factor) * icp3_ref._kth(fin, icp3_chain_ref.median_rank(len(fin))))
        keep = keep & icp3_chain_ref.ox_keep(ox, d2, med_limit)
        if trace is not None:
            trace.append((ids.copy(), d2.copy(), keep.copy()))
        if not keep.any():
            status = 2                                 # "no point to minimize"
            break
        P = np.stack([v[keep].astype(np.float64) for v in c], 1)
        q = ids[keep]
        Q = np.stack([v[q].astype(np.float64) for v in t], 1)
        A, b = system(P, Q, nv[q], reverse_sums)
        if singular(A):
            status = 5
            break
        Ts = np.eye(4)
        Ts[:3, :3], Ts[:3, 3] = step(A, b)
        Ti = mat4(Ts.astype(f32), Ti)
        iters += 1
        counter += 1
        last = counter >= p.max_iter
        out = False
        if use_bound and not ((ox.bound_order & 1) and last):
            out = icp3_chain_ref.bound_out(ox, Ti)
        if out and not (ox.bound_order & 2):
            status = 9                                 # "limit out of bounds"
            break
        iterate = not last
        if not last and p.use_diff_checker:
            hist.append(Ti.copy())
            hist = hist[-MAX_HIST:]
            if iters + 1 > p.smooth_len:
                rsum = tsum = 0.0
                for i in range(len(hist) - 1, len(hist) - 1 - p.smooth_len, -1):
                    a, bb = hist[i].astype(np.float64), hist[i - 1].astype(np.float64)
                    rsum += quat_dist(quat(a[:3, :3]), quat(bb[:3, :3]))
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
        if out and status == 0:
            status = 9
        if status != 0 or not iterate:
            break
    if status != 0:
        return status, guess.copy(), iters
    return status, mat4(icp3_ref.translate(mean), mat4(Ti, T0)), iters
