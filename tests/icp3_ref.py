"""numpy restatement of the 3-D point-to-point ICP chain of ``sfe_icp3_compute_jobs`` (include/sonarfe.h and INTEGRATION.md
state the rules): KDTreeMatcher {knn 1}, MaxDist and TrimmedDist outlier filters, PointToPointErrorMinimizer, Counter and
Differential transformation checkers.  Float32 step by step where a decision depends on it (frame, moved cloud, squared
distances, history), fp64 sums, ``np.linalg.svd`` for the rotation.  Where a rule also exists in 2-D it is
``icp_chain_ref``'s with one more coordinate.  Test infrastructure only; the product never imports it.

``reverse_sums=True`` takes the fp64 sums in reversed point order (the input-stability check of the GPU tests' inputs);
``reflection_fix=False`` leaves U V^T as the SVD hands it back (to show which inputs need the fix: the nearly planar ones)."""
import numpy as np

f32 = np.float32
MAX_HIST = 64


def mat4(a, b):
    """a @ b, 4 x 4 float32, each entry (((a0 b0 + a1 b1) + a2 b2) + a3 b3) rounded step by step (mat4_mul)"""
    a = np.asarray(a, f32).reshape(4, 4)
    b = np.asarray(b, f32).reshape(4, 4)
    r = np.zeros((4, 4), f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(4):
            for j in range(4):
                s = f32(a[i, 0] * b[0, j])
                for k in (1, 2, 3):
                    s = f32(s + f32(a[i, k] * b[k, j]))
                r[i, j] = s
    return r


def affine(T, x, y, z):
    """rows 0..2 of T applied to float32 columns: ((T0 x + T1 y) + T2 z) + T3, every step rounded"""
    T = np.asarray(T, f32).reshape(4, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        return tuple(((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] for i in range(3))


def translate(v):
    T = np.eye(4, dtype=f32)
    T[:3, 3] = v
    return T


def embed(T3):
    """a 3 x 3 planar transform as 4 x 4: rotation about z, translation in the plane"""
    T3 = np.asarray(T3, f32).reshape(3, 3)
    T = np.eye(4, dtype=f32)
    T[:2, :2] = T3[:2, :2]
    T[:2, 3] = T3[:2, 2]
    return T


def nn(c, t, r2_match, tie_high=False):
    """exact 1-NN: d2 = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)), lowest index among equals; !(d2 <= r2) -> (-1, inf)"""
    n = len(c[0])
    ids = np.empty(n, np.int64)
    d2 = np.empty(n, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, n, 256):
            dx = c[0][a:a + 256, None] - t[0][None, :]
            dy = c[1][a:a + 256, None] - t[1][None, :]
            dz = c[2][a:a + 256, None] - t[2][None, :]
            d = (dx * dx + dy * dy) + dz * dz
            d = np.where(np.isnan(d), f32(np.inf), d)          # NaN never wins, and is no match below
            j = np.argmin(d, axis=1)                           # the first index among equals
            if tie_high:
                j = d.shape[1] - 1 - np.argmin(d[:, ::-1], axis=1)
            ids[a:a + 256] = j
            d2[a:a + 256] = d[np.arange(len(j)), j]
        none = ~(d2 <= r2_match) | (d2 == np.inf)
    ids[none] = -1
    d2[none] = np.inf
    return ids, d2


def quat(m):
    """Eigen's Quaternion(Matrix3) branch rule on an fp64 3 x 3 block -> (w, x, y, z), not normalised"""
    m = np.asarray(m, np.float64).reshape(3, 3)
    q = np.zeros(4)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = m[0, 0] + m[1, 1] + m[2, 2]
        if t > 0.0:
            t = np.sqrt(t + 1.0)
            q[0] = 0.5 * t
            t = 0.5 / t
            q[1] = (m[2, 1] - m[1, 2]) * t
            q[2] = (m[0, 2] - m[2, 0]) * t
            q[3] = (m[1, 0] - m[0, 1]) * t
        else:
            i = 0
            if m[1, 1] > m[0, 0]:
                i = 1
            if m[2, 2] > m[i, i]:
                i = 2
            j = (i + 1) % 3
            k = (j + 1) % 3
            t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
            q[1 + i] = 0.5 * t
            t = 0.5 / t
            q[0] = (m[k, j] - m[j, k]) * t
            q[1 + j] = (m[j, i] + m[i, j]) * t
            q[1 + k] = (m[k, i] + m[i, k]) * t
    return q


def quat_dist(a, b):
    """Eigen's angularDistance: 2 atan2(|vec(a * conj(b))|, |w|)"""
    bw, bx, by, bz = b[0], -b[1], -b[2], -b[3]
    w = a[0] * bw - a[1] * bx - a[2] * by - a[3] * bz
    x = a[0] * bx + a[1] * bw + a[2] * bz - a[3] * by
    y = a[0] * by + a[2] * bw + a[3] * bx - a[1] * bz
    z = a[0] * bz + a[3] * bw + a[1] * by - a[2] * bx
    return 2.0 * np.arctan2(np.sqrt(x * x + y * y + z * z), abs(w))


def rotation(H, reflection_fix=True, stats=None):
    """the proper rotation closest to H: U V^T, the column of U of the smallest singular value negated when det < 0
    (``stats["reflections"]`` counts how often)"""
    U, _, Vt = np.linalg.svd(H)
    R = U @ Vt
    if np.linalg.det(R) < 0:
        if stats is not None:
            stats["reflections"] = stats.get("reflections", 0) + 1
        if reflection_fix:
            U = U.copy()
            U[:, 2] = -U[:, 2]
            R = U @ Vt
    return R


def solve(acc, reflection_fix=True, stats=None):
    """the 16 sums (W, sum p, sum q, sum q p^T row-major) -> (R, t)"""
    W = acc[0]
    sp, sq, A = acc[1:4], acc[4:7], acc[7:16].reshape(3, 3)
    mp, mq = sp / W, sq / W
    H = A - np.outer(sq, mp)
    R = rotation(H, reflection_fix, stats)
    t = np.array([mq[i] - ((R[i, 0] * mp[0] + R[i, 1] * mp[1]) + R[i, 2] * mp[2]) for i in range(3)])
    return R, t


def _kth(fin, k):
    return f32(np.partition(fin, k)[k])


def icp(src, tgt, guess, p, reverse_sums=False, reflection_fix=True, trace=None, tie_high=False, stats=None):
    """-> (status, T 4 x 4 float32, iterations) of one job.  p: IcpParams (or an object with its fields), minimizer 0.
    ``trace``: a list that receives (ids, d2, keep) of every iteration; ``tie_high``: the matcher takes the HIGHEST index
    among equal distances (the wrong rule, to show that an input depends on the right one); ``stats``: a dict that counts
    the steps whose U V^T was a reflection."""
    assert p.minimizer == 0
    src = np.ascontiguousarray(src, f32).reshape(-1, 3)
    tgt = np.ascontiguousarray(tgt, f32).reshape(-1, 3)
    guess = np.asarray(guess, f32).reshape(4, 4)
    nt = len(tgt)
    with np.errstate(invalid="ignore", over="ignore"):
        mean = np.array([f32(np.cumsum(tgt[:, a].astype(np.float64))[-1] / nt) for a in range(3)], f32)
        t = tuple(tgt[:, a] - mean[a] for a in range(3))
    T0 = mat4(translate(-mean), guess)
    r = affine(T0, src[:, 0], src[:, 1], src[:, 2])
    r2_match = f32(f32(p.matcher_max_dist) * f32(p.matcher_max_dist))
    r2_filter = f32(f32(p.max_dist_filter) * f32(p.max_dist_filter))
    Ti = np.eye(4, dtype=f32)
    hist = [Ti.copy()]                                 # DifferentialTransformationChecker::init: the identity
    status, iters, counter = 0, 0, 0
    while True:
        c = affine(Ti, *r)
        ids, d2 = nn(c, t, r2_match, tie_high)
        keep = ids >= 0
        fin = d2[keep]
        if p.use_max_dist_filter:
            keep = keep & (d2 <= r2_filter)
        if p.use_trimmed_filter:
            if len(fin) == 0:
                status = 1                             # "no outlier to filter"
                break
            k = len(fin) - 1 if p.trim_ratio >= 1.0 else int(f32(len(fin)) * f32(p.trim_ratio))
            keep = keep & (d2 <= _kth(fin, k))
        if trace is not None:
            trace.append((ids.copy(), d2.copy(), keep.copy()))
        if not keep.any():
            status = 2                                 # "no point to minimize"
            break
        P = np.stack([v[keep].astype(np.float64) for v in c], 1)
        q = ids[keep]
        Q = np.stack([v[q].astype(np.float64) for v in t], 1)
        if reverse_sums:
            P, Q = P[::-1], Q[::-1]
        acc = np.zeros(16)
        acc[0] = float(keep.sum())
        acc[1:4] = [np.cumsum(P[:, a])[-1] for a in range(3)]
        acc[4:7] = [np.cumsum(Q[:, a])[-1] for a in range(3)]
        acc[7:16] = [np.cumsum(Q[:, i] * P[:, j])[-1] for i in range(3) for j in range(3)]
        R, tr = solve(acc, reflection_fix, stats)
        Ts = np.eye(4)
        Ts[:3, :3] = R
        Ts[:3, 3] = tr
        Ti = mat4(Ts.astype(f32), Ti)
        iters += 1
        counter += 1
        iterate = True
        if counter >= p.max_iter:
            iterate = False                            # CounterTransformationChecker
        elif p.use_diff_checker:
            hist.append(Ti.copy())
            hist = hist[-MAX_HIST:]                    # a sliding window (only the last smooth_len + 1 entries are read)
            if iters + 1 > p.smooth_len:
                rsum = tsum = 0.0
                for i in range(len(hist) - 1, len(hist) - 1 - p.smooth_len, -1):
                    a, b = hist[i].astype(np.float64), hist[i - 1].astype(np.float64)
                    rsum += quat_dist(quat(a[:3, :3]), quat(b[:3, :3]))
                    d = a[:3, 3] - b[:3, 3]
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
    return status, mat4(translate(mean), mat4(Ti, T0)), iters
