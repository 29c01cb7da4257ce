// The one-lane arithmetic of the 3-D point-to-point ICP (sfe_icp3.hip), plain C++ in fp64 so that the CPU can check it
// (tests/host/icp3_solve_check.cpp): the error minimiser's solve, reduced sums -> (R, t), and the rotation distance of
// the DifferentialTransformationChecker.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define SFE_ICP3_HD __host__ __device__ inline
#define SFE_ICP3_UNROLL _Pragma("unroll") // the matrices stay in registers only if every index is a constant
#else
#define SFE_ICP3_HD inline
#define SFE_ICP3_UNROLL
#endif

#define ICP3_NSUM 16          // W, sum p (3), sum q (3), sum q p^T (9, row-major: [7 + 3 i + j] = sum q_i p_j)
#define ICP3_JACOBI_SWEEPS 12 // cyclic Jacobi sweeps over the 4 x 4 matrix, at most (quadratic convergence; it ends earlier)

// Eigenvectors of the symmetric 4 x 4 matrix a (overwritten; its diagonal ends as the eigenvalues) as the columns of v:
// cyclic Jacobi, a fixed number of sweeps at most, no division by a zero pivot; non-finite input ends with non-finite
// output, never in an endless loop.
SFE_ICP3_HD void icp3_jacobi4(double (&a)[4][4], double (&v)[4][4])
{
    SFE_ICP3_UNROLL
    for (int i = 0; i < 4; ++i)
        SFE_ICP3_UNROLL
        for (int j = 0; j < 4; ++j)
            v[i][j] = (i == j) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < ICP3_JACOBI_SWEEPS; ++sweep) {
        double off = 0, diag = 0;
        SFE_ICP3_UNROLL
        for (int i = 0; i < 4; ++i) {
            diag += a[i][i] * a[i][i];
            SFE_ICP3_UNROLL
            for (int j = i + 1; j < 4; ++j)
                off += a[i][j] * a[i][j];
        }
        if (off <= 1e-36 * diag) // off-diagonal below 1e-18 of the diagonal (also off == 0; NaN: goes on, the sweeps are counted)
            break;
        SFE_ICP3_UNROLL
        for (int p = 0; p < 3; ++p)
            SFE_ICP3_UNROLL
            for (int q = p + 1; q < 4; ++q) {
                const double apq = a[p][q];
                if (apq == 0.0)
                    continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                SFE_ICP3_UNROLL
                for (int k = 0; k < 4; ++k) { // columns p, q of a and of v
                    const double akp = a[k][p], akq = a[k][q];
                    a[k][p] = c * akp - s * akq;
                    a[k][q] = s * akp + c * akq;
                    const double vkp = v[k][p], vkq = v[k][q];
                    v[k][p] = c * vkp - s * vkq;
                    v[k][q] = s * vkp + c * vkq;
                }
                SFE_ICP3_UNROLL
                for (int k = 0; k < 4; ++k) { // rows p, q of a
                    const double apk = a[p][k], aqk = a[q][k];
                    a[p][k] = c * apk - s * aqk;
                    a[q][k] = s * apk + c * aqk;
                }
            }
    }
}

// The proper rotation closest to H (3 x 3, row-major; H = sum (q - mq)(p - mp)^T, q the reference points): the R that
// maximises trace(R^T H), det R = +1 -- U V^T of the SVD H = U S V^T with the column of U of the smallest singular value
// negated where det(U V^T) < 0.  Taken as the eigenvector of the largest eigenvalue of Horn's symmetric 4 x 4 matrix (a unit
// quaternion, so always a proper rotation, without a reflection branch).  H of rank <= 1 leaves R undetermined: some
// rotation comes back (the identity for H = 0), finite for finite H.
SFE_ICP3_HD void icp3_rotation(const double *H, double *R)
{
    // S_ab = sum p_a q_b = H[b][a]
    const double Sxx = H[0], Sxy = H[3], Sxz = H[6];
    const double Syx = H[1], Syy = H[4], Syz = H[7];
    const double Szx = H[2], Szy = H[5], Szz = H[8];
    double a[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
    double v[4][4];
    icp3_jacobi4(a, v);
    // the column of the largest eigenvalue (the first among equals), picked without a variable index
    double top = a[0][0], w = v[0][0], x = v[1][0], y = v[2][0], z = v[3][0];
    SFE_ICP3_UNROLL
    for (int i = 1; i < 4; ++i)
        if (a[i][i] > top) {
            top = a[i][i];
            w = v[0][i];
            x = v[1][i];
            y = v[2][i];
            z = v[3][i];
        }
    const double n = sqrt(w * w + x * x + y * y + z * z);
    w /= n;
    x /= n;
    y /= n;
    z /= n;
    R[0] = 1.0 - 2.0 * (y * y + z * z);
    R[1] = 2.0 * (x * y - w * z);
    R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);
    R[4] = 1.0 - 2.0 * (x * x + z * z);
    R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);
    R[7] = 2.0 * (y * z + w * x);
    R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// PointToPointErrorMinimizer in 3-D from the fp64 sums over the kept pairs (acc[0] = W > 0): mp = sum p / W, mq = sum q / W,
// H = sum q p^T - (sum q) mp^T (the expression shape of the 2-D solve), R = icp3_rotation(H), t = mq - R mp.
SFE_ICP3_HD void icp3_solve(const double *acc, double *R, double *t)
{
    const double W = acc[0];
    const double mp[3] = {acc[1] / W, acc[2] / W, acc[3] / W};
    const double mq[3] = {acc[4] / W, acc[5] / W, acc[6] / W};
    double H[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            H[3 * i + j] = acc[7 + 3 * i + j] - acc[4 + i] * mp[j];
    icp3_rotation(H, R);
    for (int i = 0; i < 3; ++i)
        t[i] = mq[i] - ((R[3 * i] * mp[0] + R[3 * i + 1] * mp[1]) + R[3 * i + 2] * mp[2]);
}

// Quaternion (w, x, y, z) of the 3 x 3 block m (row-major) by the branch rule of Eigen's Quaternion(Matrix3): trace > 0,
// else the largest diagonal entry (the first among equals); not normalised, like Eigen's.
SFE_ICP3_HD void icp3_quat(const double *m, double *q)
{
    double t = m[0] + m[4] + m[8];
    if (t > 0.0) {
        t = sqrt(t + 1.0);
        q[0] = 0.5 * t;
        t = 0.5 / t;
        q[1] = (m[7] - m[5]) * t;
        q[2] = (m[2] - m[6]) * t;
        q[3] = (m[3] - m[1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0])
            i = 1;
        if (m[8] > m[4 * i])
            i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0);
        q[1 + i] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[3 * k + j] - m[3 * j + k]) * t;
        q[1 + j] = (m[3 * j + i] + m[3 * i + j]) * t;
        q[1 + k] = (m[3 * k + i] + m[3 * i + k]) * t;
    }
}

// Eigen's Quaternion::angularDistance: 2 atan2(|vec(d)|, |d.w|) with d = a * conj(b)
SFE_ICP3_HD double icp3_quat_dist(const double *a, const double *b)
{
    const double bw = b[0], bx = -b[1], by = -b[2], bz = -b[3];
    const double w = a[0] * bw - a[1] * bx - a[2] * by - a[3] * bz;
    const double x = a[0] * bx + a[1] * bw + a[2] * bz - a[3] * by;
    const double y = a[0] * by + a[2] * bw + a[3] * bx - a[1] * bz;
    const double z = a[0] * bz + a[3] * bw + a[1] * by - a[2] * bx;
    return 2.0 * atan2(sqrt(x * x + y * y + z * z), fabs(w));
}

// rotation distance of two float 3 x 3 blocks (row-major), in fp64 from the floats
SFE_ICP3_HD double icp3_rot_dist(const float *ma, const float *mb)
{
    double a[9], b[9], qa[4], qb[4];
    for (int i = 0; i < 9; ++i) {
        a[i] = ma[i];
        b[i] = mb[i];
    }
    icp3_quat(a, qa);
    icp3_quat(b, qb);
    return icp3_quat_dist(qa, qb);
}
