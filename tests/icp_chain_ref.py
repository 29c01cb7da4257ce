"""numpy restatement of the ICP loop of a chain with the outlier filters and the checker of ``sfe_icp_outliers``
(MinDist, MedianDist, Bound; include/sonarfe.h states their rules) next to those of ``sfe_icp_params``.  Float
operations are the oracle's (every product and sum rounded to float32, exact 1-NN with the lowest index on ties); the
error minimiser's sums are fp64, like the oracle's fp64-sum mode and the kernels (in another order: poses agree to
rounding, not bit for bit).  Test infrastructure only; the product never imports it."""
import numpy as np

import oracle

f32 = np.float32
PIVOT_RTOL = 1e-10


def _mat3(a, b):
    """a @ b, 3 x 3 float32, each entry ((a0 b0 + a1 b1) + a2 b2) rounded step by step (mat3_mul)"""
    a = np.asarray(a, f32).reshape(3, 3)
    b = np.asarray(b, f32).reshape(3, 3)
    r = np.zeros((3, 3), f32)
    for i in range(3):
        for j in range(3):
            s = f32(a[i, 0] * b[0, j])
            s = f32(s + f32(a[i, 1] * b[1, j]))
            s = f32(s + f32(a[i, 2] * b[2, j]))
            r[i, j] = s
    return r


def _affine(T, x, y):
    """((T0 x + T1 y) + T2, (T3 x + T4 y) + T5) in float32"""
    t = T.reshape(-1)
    return (f32(t[0]) * x + f32(t[1]) * y) + f32(t[2]), (f32(t[3]) * x + f32(t[4]) * y) + f32(t[5])


def _nn(cx, cy, tx, ty, r2_match):
    """exact 1-NN: d2 = fl(fl(dx dx) + fl(dy dy)), lowest index among equals; no match -> (-1, inf)"""
    ids = np.empty(len(cx), np.int64)
    d2 = np.empty(len(cx), f32)
    for a in range(0, len(cx), 512):
        dx = cx[a:a + 512, None] - tx[None, :]
        dy = cy[a:a + 512, None] - ty[None, :]
        d = dx * dx + dy * dy
        j = np.argmin(d, axis=1)
        ids[a:a + 512] = j
        d2[a:a + 512] = d[np.arange(len(j)), j]
    none = ~(d2 <= r2_match) | (d2 == np.inf)
    ids[none] = -1
    d2[none] = np.inf
    return ids, d2


def _kth(fin, k):
    return f32(np.partition(fin, k)[k])


def icp(src, tgt, guess, p, ox=None):
    """-> (status, T 3 x 3 float32, iterations) of one job.  p: IcpParams (or an object with its fields), ox:
    IcpOutliers or None."""
    src = np.ascontiguousarray(src, f32).reshape(-1, 2)
    tgt = np.ascontiguousarray(tgt, f32).reshape(-1, 2)
    guess = np.asarray(guess, f32).reshape(3, 3)
    use_min = bool(ox and ox.use_min_dist)
    use_med = bool(ox and ox.use_median)
    use_bound = bool(ox and ox.use_bound)
    # reference mean: fp64 sum in point order, rounded to float; the centred reference
    nt = len(tgt)
    mx = f32(np.cumsum(tgt[:, 0].astype(np.float64))[-1] / nt)
    my = f32(np.cumsum(tgt[:, 1].astype(np.float64))[-1] / nt)
    tx, ty = tgt[:, 0] - mx, tgt[:, 1] - my
    nrm = oracle.normals2d(np.stack([tx, ty], 1), p.normals_knn) if p.minimizer == 1 else None
    T0 = _mat3(np.array([[1, 0, -mx], [0, 1, -my], [0, 0, 1]], f32), guess)
    rx, ry = _affine(T0, src[:, 0], src[:, 1])
    r2_match = f32(f32(p.matcher_max_dist) * f32(p.matcher_max_dist))
    r2_filter = f32(f32(p.max_dist_filter) * f32(p.max_dist_filter))
    min2 = f32(f32(ox.min_dist) * f32(ox.min_dist)) if use_min else f32(0)
    Ti = np.eye(3, dtype=f32)
    hist = [(f32(1), f32(0), f32(0), f32(0))]       # DifferentialTransformationChecker::init: the identity
    status, iters, counter = 0, 0, 0
    while True:
        cx, cy = _affine(Ti, rx, ry)
        ids, d2 = _nn(cx, cy, tx, ty, r2_match)
        fin = d2[ids >= 0]
        keep = ids >= 0
        if p.use_max_dist_filter:
            keep &= d2 <= r2_filter
        if (p.use_trimmed_filter or use_med) and len(fin) == 0:
            status = 1                                 # "no outlier to filter"
            break
        if p.use_trimmed_filter:
            k = len(fin) - 1 if p.trim_ratio >= 1.0 else int(f32(len(fin)) * f32(p.trim_ratio))
            keep &= d2 <= _kth(fin, k)
        if use_min:
            keep &= d2 >= min2
        if use_med:
            med = _kth(fin, int(f32(len(fin)) * f32(0.5)))
            keep &= d2 <= f32(f32(ox.median_factor) * med)
        if not keep.any():
            status = 2                                 # "no point to minimize"
            break
        px, py = cx[keep].astype(np.float64), cy[keep].astype(np.float64)
        q = ids[keep]
        qx, qy = tx[q].astype(np.float64), ty[q].astype(np.float64)
        if p.minimizer == 0:
            W = float(keep.sum())
            spx, spy, sqx, sqy = px.sum(), py.sum(), qx.sum(), qy.sum()
            a00, a01, a10, a11 = (qx * px).sum(), (qx * py).sum(), (qy * px).sum(), (qy * py).sum()
            mpx, mpy, mqx, mqy = spx / W, spy / W, sqx / W, sqy / W
            m00, m01 = a00 - sqx * mpx, a01 - sqx * mpy
            m10, m11 = a10 - sqy * mpx, a11 - sqy * mpy
            S, K = m00 + m11, m10 - m01
            h = np.sqrt(S * S + K * K)
            c, s = (1.0, 0.0) if h == 0 else (S / h, K / h)
            t0, t1 = mqx - (c * mpx - s * mpy), mqy - (s * mpx + c * mpy)
        else:
            nx, ny = nrm[q, 0].astype(np.float64), nrm[q, 1].astype(np.float64)
            a0 = px * ny - py * nx
            e = nx * (px - qx) + ny * (py - qy)
            A = [(a0 * a0).sum(), (a0 * nx).sum(), (a0 * ny).sum(), (nx * nx).sum(), (nx * ny).sum(), (ny * ny).sum()]
            B = [-(a0 * e).sum(), -(nx * e).sum(), -(ny * e).sum()]
            with np.errstate(invalid="ignore", divide="ignore"):
                l00 = np.sqrt(A[0])
                l10, l20 = A[1] / l00, A[2] / l00
                p11 = A[3] - l10 * l10
                l11 = np.sqrt(p11)
                l21 = (A[4] - l20 * l10) / l11
                p22 = A[5] - l20 * l20 - l21 * l21
                l22 = np.sqrt(p22)
            if not (l00 > 0) or not (p11 > PIVOT_RTOL * A[3]) or not (p22 > PIVOT_RTOL * A[5]):
                status = 5
                break
            y0 = B[0] / l00
            y1 = (B[1] - l10 * y0) / l11
            y2 = (B[2] - l20 * y0 - l21 * y1) / l22
            x2 = y2 / l22
            x1 = (y1 - l21 * x2) / l11
            x0 = (y0 - l10 * x1 - l20 * x2) / l00
            c, s, t0, t1 = np.cos(x0), np.sin(x0), x1, x2
        Ts = np.array([[c, -s, t0], [s, c, t1], [0, 0, 1]], np.float64).astype(f32)
        Ti = _mat3(Ts, Ti)
        iters += 1
        counter += 1
        last = counter >= p.max_iter
        out = False
        if use_bound and not ((ox.bound_order & 1) and last):
            with np.errstate(invalid="ignore"):
                rot = np.arccos(Ti[0, 0])
            tr = np.sqrt(f32(f32(Ti[0, 2] * Ti[0, 2]) + f32(Ti[1, 2] * Ti[1, 2])))
            out = bool(rot > f32(ox.max_rotation_norm) or tr > f32(ox.max_translation_norm))
        if out and not (ox.bound_order & 2):
            status = 9                                 # "limit out of bounds"
            break
        iterate = not last
        if not last and p.use_diff_checker:
            hist.append((Ti[0, 0], Ti[1, 0], Ti[0, 2], Ti[1, 2]))
            if len(hist) > p.smooth_len:
                rsum = tsum = 0.0
                for i in range(len(hist) - 1, len(hist) - 1 - p.smooth_len, -1):
                    c1, s1, x1_, y1_ = (float(v) for v in hist[i])
                    c0, s0, x0_, y0_ = (float(v) for v in hist[i - 1])
                    rsum += abs(np.arctan2(s1 * c0 - c1 * s0, c1 * c0 + s1 * s0))
                    tsum += np.sqrt((x1_ - x0_) ** 2 + (y1_ - y0_) ** 2)
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
    T = _mat3(np.array([[1, 0, mx], [0, 1, my], [0, 0, 1]], f32), _mat3(Ti, T0))
    return status, T, iters
