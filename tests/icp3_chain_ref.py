"""numpy restatement of the 3-D ICP loop of a chain with the modules of ``sfe_icp_outliers`` (MinDist, MedianDist, Bound;
include/sonarfe.h states their rules at ``sfe_icp3_compute_jobs_chain_ext``): the loop of ``icp3_ref.icp`` (minimizer 0) /
``icp3_plane_ref.icp`` (minimizer 2), whose ``mat4``, ``nn``, ``solve``, ``quat`` and ``quat_dist`` it imports, with the
extra outlier filters in the keep test and the Bound checker in its place among the checkers (``icp_chain_ref``'s rule).
Test infrastructure only; the product never imports it.

Wrong variants, to show that an input depends on the right rule (``wrong=`` one of them):
  "min_strict"    MinDist keeps d2 >  minDist^2 (the rule is >=)
  "median_all"    the median is taken over all d2, the infinite ones of unmatched queries included (the rule: the finite ones)
  "bound_first"   Bound is evaluated before the Counter whatever the listed order (the rule: a Counter listed before it
                  that reaches its limit ends the job first)"""
import numpy as np

import icp3_plane_ref
import icp3_ref
from icp3_ref import MAX_HIST, f32, mat4, nn, quat, quat_dist, solve

WRONG = ("min_strict", "median_all", "bound_first")


def bound_rot(T):
    """the Bound checker's rotation: the quaternion angle between T's float rotation block and the identity, fp64"""
    return quat_dist(quat(np.asarray(T, f32).reshape(4, 4)[:3, :3].astype(np.float64)), quat(np.eye(3)))


def bound_trans(T):
    t = np.asarray(T, f32).reshape(4, 4)[:3, 3].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])


def bound_out(ox, T):
    """out of bounds?  (a NaN never is)"""
    with np.errstate(invalid="ignore"):
        return bool(bound_rot(T) > float(f32(ox.max_rotation_norm)) or bound_trans(T) > float(f32(ox.max_translation_norm)))


def median_rank(n):
    return int(f32(n) * f32(0.5))


def ox_keep(ox, d2, med_limit, wrong=None):
    """bool [N]: the pairs MinDist and MedianDist keep (med_limit: fl(factor x median), unused without MedianDist)"""
    keep = np.ones(len(d2), bool)
    if ox is not None and ox.use_min_dist:
        min2 = f32(f32(ox.min_dist) * f32(ox.min_dist))
        keep &= (d2 > min2) if wrong == "min_strict" else (d2 >= min2)
    if ox is not None and ox.use_median:
        keep &= d2 <= med_limit
    return keep


def icp(src, tgt, guess, p, ox=None, wrong=None, trace=None, normals_of=None):
    """-> (status, T 4 x 4 float32, iterations) of one job.  p: IcpParams with minimizer 0 or 2, ox: IcpOutliers or None.
    ``trace``: a list that receives (ids, d2, keep) of every iteration."""
    assert p.minimizer in (0, 2) and wrong in (None,) + WRONG
    src = np.ascontiguousarray(src, f32).reshape(-1, 3)
    tgt = np.ascontiguousarray(tgt, f32).reshape(-1, 3)
    guess = np.asarray(guess, f32).reshape(4, 4)
    use_med = bool(ox is not None and ox.use_median)
    use_bound = bool(ox is not None and ox.use_bound)
    mean, t = icp3_plane_ref.centred(tgt)
    nv = None
    if p.minimizer == 2:
        nv = normals_of if normals_of is not None else icp3_plane_ref.normals(tgt, p.normals_knn, centre=True)
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
            pool = d2 if wrong == "median_all" else fin
            med_limit = f32(f32(ox.median_factor) * icp3_ref._kth(pool, median_rank(len(pool))))
        keep = keep & ox_keep(ox, d2, med_limit, wrong)
        if trace is not None:
            trace.append((ids.copy(), d2.copy(), keep.copy()))
        if not keep.any():
            status = 2                                 # "no point to minimize"
            break
        P = np.stack([v[keep].astype(np.float64) for v in c], 1)
        q = ids[keep]
        Q = np.stack([v[q].astype(np.float64) for v in t], 1)
        Ts = np.eye(4)
        if p.minimizer == 0:
            acc = np.zeros(16)
            acc[0] = float(keep.sum())
            acc[1:4] = [np.cumsum(P[:, a])[-1] for a in range(3)]
            acc[4:7] = [np.cumsum(Q[:, a])[-1] for a in range(3)]
            acc[7:16] = [np.cumsum(Q[:, i] * P[:, j])[-1] for i in range(3) for j in range(3)]
            Ts[:3, :3], Ts[:3, 3] = solve(acc)
        else:
            A, b = icp3_plane_ref.system(P, Q, nv[q])
            if icp3_plane_ref.singular(A):
                status = 5
                break
            x = np.linalg.solve(A, b)
            Ts[:3, :3] = icp3_plane_ref.rodrigues(x[:3])
            Ts[:3, 3] = x[3:]
        Ti = mat4(Ts.astype(f32), Ti)
        iters += 1
        counter += 1
        last = counter >= p.max_iter
        out = False
        if use_bound and not ((ox.bound_order & 1) and last and wrong != "bound_first"):
            out = bound_out(ox, Ti)
        if out and (not (ox.bound_order & 2) or wrong == "bound_first"):
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
