// The one-lane arithmetic of the 3-D point-to-plane ICP (sfe_icp3.hip, sfe_icp_params.minimizer == 2), plain C++ in fp64 so
// that the CPU can check it (tests/host/icp3_plane_check.cpp): the surface normal of a neighbourhood (3 x 3 symmetric
// Jacobi, eigenvector of the smallest eigenvalue), the 6 x 6 Cholesky solve of the normal equations with the 2-D
// minimiser's singularity rule, and Rodrigues' rotation; for minimizer == 3 (force4DOF: 1: yaw and translation only) the
// 4 x 4 solve under the same rule and the rotation about z.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define SFE_ICP3P_HD __host__ __device__ inline
#define SFE_ICP3P_UNROLL _Pragma("unroll") // the matrices stay in registers only if every index is a constant
#else
#define SFE_ICP3P_HD inline
#define SFE_ICP3P_UNROLL
#endif

#define ICP3P_NSUM 28          // W, A = sum F F^T (21: the upper triangle row by row), b = -sum F e (6)
#define ICP3P4_NSUM 15         // force4DOF: W, A = sum F F^T (10) and b = -sum F e (4) with F = ((p x n)_z, n)
#define ICP3P_JACOBI_SWEEPS 12 // cyclic Jacobi sweeps over the 3 x 3 matrix, at most (quadratic convergence; it ends earlier)
#define ICP3P_PIVOT_RTOL 1e-10 // ICP_PIVOT_RTOL of the 2-D minimiser (sfe_icp_common.h)

// Eigenvectors of the symmetric 3 x 3 matrix a (overwritten; its diagonal ends as the eigenvalues) as the columns of v: cyclic
// Jacobi over (0,1), (0,2), (1,2), a fixed number of sweeps at most, a sweep is skipped once the off-diagonal part is below
// 1e-18 of the diagonal; no division by a zero pivot; non-finite input ends with non-finite output, never in an endless loop.
SFE_ICP3P_HD void icp3p_jacobi3(double (&a)[3][3], double (&v)[3][3])
{
    SFE_ICP3P_UNROLL
    for (int i = 0; i < 3; ++i)
        SFE_ICP3P_UNROLL
        for (int j = 0; j < 3; ++j)
            v[i][j] = (i == j) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < ICP3P_JACOBI_SWEEPS; ++sweep) {
        double off = 0, diag = 0;
        SFE_ICP3P_UNROLL
        for (int i = 0; i < 3; ++i) {
            diag += a[i][i] * a[i][i];
            SFE_ICP3P_UNROLL
            for (int j = i + 1; j < 3; ++j)
                off += a[i][j] * a[i][j];
        }
        if (off <= 1e-36 * diag) // (also off == 0; NaN: goes on, the sweeps are counted)
            break;
        SFE_ICP3P_UNROLL
        for (int p = 0; p < 2; ++p)
            SFE_ICP3P_UNROLL
            for (int q = p + 1; q < 3; ++q) {
                const double apq = a[p][q];
                if (apq == 0.0)
                    continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                SFE_ICP3P_UNROLL
                for (int k = 0; k < 3; ++k) { // columns p, q of a and of v
                    const double akp = a[k][p], akq = a[k][q];
                    a[k][p] = c * akp - s * akq;
                    a[k][q] = s * akp + c * akq;
                    const double vkp = v[k][p], vkq = v[k][q];
                    v[k][p] = c * vkp - s * vkq;
                    v[k][q] = s * vkp + c * vkq;
                }
                SFE_ICP3P_UNROLL
                for (int k = 0; k < 3; ++k) { // rows p, q of a
                    const double apk = a[p][k], aqk = a[q][k];
                    a[p][k] = c * apk - s * aqk;
                    a[q][k] = s * apk + c * aqk;
                }
            }
    }
}

// The surface normal of a neighbourhood from its scatter matrix C = sum (u - m)(u - m)^T (row-major, symmetric): the unit
// eigenvector of the smallest eigenvalue, the lowest column among equal eigenvalues, its sign as the Jacobi leaves it.
// Always a finite unit vector: C = 0 gives (1, 0, 0) (the Jacobi does not turn), and so does a C that is not finite.
SFE_ICP3P_HD void icp3p_normal(const double *C, double *n)
{
    // scaled by its largest entry first (the eigenvectors stay): the Jacobi's stopping rule squares the entries
    double big = 0.0;
    SFE_ICP3P_UNROLL
    for (int i = 0; i < 9; ++i)
        big = fabs(C[i]) > big ? fabs(C[i]) : big; // (NaN: never the larger)
    const double sc = (big > 0.0 && big < INFINITY) ? 1.0 / big : 1.0;
    double a[3][3] = {{C[0] * sc, C[1] * sc, C[2] * sc}, {C[1] * sc, C[4] * sc, C[5] * sc}, {C[2] * sc, C[5] * sc, C[8] * sc}};
    double v[3][3];
    icp3p_jacobi3(a, v);
    // the column of the smallest eigenvalue (the first among equals), picked without a variable index
    double low = a[0][0], x = v[0][0], y = v[1][0], z = v[2][0];
    SFE_ICP3P_UNROLL
    for (int i = 1; i < 3; ++i)
        if (a[i][i] < low) {
            low = a[i][i];
            x = v[0][i];
            y = v[1][i];
            z = v[2][i];
        }
    const double len = sqrt((x * x + y * y) + z * z);
    if (!(len > 0.0) || !(len < INFINITY)) { // NaN, infinite or zero
        n[0] = 1.0;
        n[1] = 0.0;
        n[2] = 0.0;
        return;
    }
    n[0] = x / len;
    n[1] = y / len;
    n[2] = z / len;
}

// A x = b for the symmetric 6 x 6 matrix whose upper triangle is A21 (row by row: 00 01 .. 05 11 12 .. 55) by a Cholesky
// factorisation, with the singularity rule of the 2-D point-to-plane minimiser (icp_solve_and_check, sfe_icp_common.h):
// A00 > 0, and every later pivot above ICP3P_PIVOT_RTOL times its diagonal entry (a pivot that has lost ten digits against
// its diagonal entry is zero in exact arithmetic and summation-order noise in floating point).  -> 0 and x, or 1 (singular,
// NaN included; x untouched).
SFE_ICP3P_HD int icp3p_chol6(const double *A21, const double *b, double *x)
{
    double L[6][6];
    {
        int k = 0;
        SFE_ICP3P_UNROLL
        for (int i = 0; i < 6; ++i)
            SFE_ICP3P_UNROLL
            for (int j = i; j < 6; ++j) {
                L[j][i] = A21[k]; // the lower triangle holds A, then the factor
                ++k;
            }
    }
    int singular = 0;
    SFE_ICP3P_UNROLL
    for (int j = 0; j < 6; ++j) {
        const double ajj = L[j][j];
        double piv = ajj;
        SFE_ICP3P_UNROLL
        for (int k = 0; k < j; ++k)
            piv -= L[j][k] * L[j][k];
        if (j == 0 ? !(piv > 0) : !(piv > ICP3P_PIVOT_RTOL * ajj))
            singular = 1;
        const double ljj = sqrt(piv);
        L[j][j] = ljj;
        SFE_ICP3P_UNROLL
        for (int i = j + 1; i < 6; ++i) {
            double s = L[i][j];
            SFE_ICP3P_UNROLL
            for (int k = 0; k < j; ++k)
                s -= L[i][k] * L[j][k];
            L[i][j] = s / ljj;
        }
    }
    if (singular)
        return 1;
    double y[6];
    SFE_ICP3P_UNROLL
    for (int i = 0; i < 6; ++i) {
        double s = b[i];
        SFE_ICP3P_UNROLL
        for (int k = 0; k < i; ++k)
            s -= L[i][k] * y[k];
        y[i] = s / L[i][i];
    }
    SFE_ICP3P_UNROLL
    for (int i = 5; i >= 0; --i) {
        double s = y[i];
        SFE_ICP3P_UNROLL
        for (int k = i + 1; k < 6; ++k)
            s -= L[k][i] * x[k];
        x[i] = s / L[i][i];
    }
    return 0;
}

// Rodrigues: the rotation by theta = |r| about r / theta, R = I + sin(theta) K + (1 - cos(theta)) K^2 (row-major);
// theta == 0 (also where the squares underflow) gives the identity, no division.
SFE_ICP3P_HD void icp3p_rodrigues(const double *r, double *R)
{
    const double theta = sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
    if (theta == 0.0) {
        R[0] = R[4] = R[8] = 1.0;
        R[1] = R[2] = R[3] = R[5] = R[6] = R[7] = 0.0;
        return;
    }
    const double kx = r[0] / theta, ky = r[1] / theta, kz = r[2] / theta;
    const double s = sin(theta), v = 1.0 - cos(theta);
    R[0] = 1.0 - v * (ky * ky + kz * kz);
    R[1] = v * (kx * ky) - s * kz;
    R[2] = v * (kx * kz) + s * ky;
    R[3] = v * (kx * ky) + s * kz;
    R[4] = 1.0 - v * (kx * kx + kz * kz);
    R[5] = v * (ky * kz) - s * kx;
    R[6] = v * (kx * kz) - s * ky;
    R[7] = v * (ky * kz) + s * kx;
    R[8] = 1.0 - v * (kx * kx + ky * ky);
}

// A x = b for the symmetric 4 x 4 matrix whose upper triangle is A10 (row by row: 00 01 02 03 11 12 13 22 23 33): icp3p_chol6
// with two rows fewer, the same singularity rule.  -> 0 and x, or 1 (singular, NaN included; x untouched).
SFE_ICP3P_HD int icp3p_chol4(const double *A10, const double *b, double *x)
{
    double L[4][4];
    {
        int k = 0;
        SFE_ICP3P_UNROLL
        for (int i = 0; i < 4; ++i)
            SFE_ICP3P_UNROLL
            for (int j = i; j < 4; ++j) {
                L[j][i] = A10[k]; // the lower triangle holds A, then the factor
                ++k;
            }
    }
    int singular = 0;
    SFE_ICP3P_UNROLL
    for (int j = 0; j < 4; ++j) {
        const double ajj = L[j][j];
        double piv = ajj;
        SFE_ICP3P_UNROLL
        for (int k = 0; k < j; ++k)
            piv -= L[j][k] * L[j][k];
        if (j == 0 ? !(piv > 0) : !(piv > ICP3P_PIVOT_RTOL * ajj))
            singular = 1;
        const double ljj = sqrt(piv);
        L[j][j] = ljj;
        SFE_ICP3P_UNROLL
        for (int i = j + 1; i < 4; ++i) {
            double s = L[i][j];
            SFE_ICP3P_UNROLL
            for (int k = 0; k < j; ++k)
                s -= L[i][k] * L[j][k];
            L[i][j] = s / ljj;
        }
    }
    if (singular)
        return 1;
    double y[4];
    SFE_ICP3P_UNROLL
    for (int i = 0; i < 4; ++i) {
        double s = b[i];
        SFE_ICP3P_UNROLL
        for (int k = 0; k < i; ++k)
            s -= L[i][k] * y[k];
        y[i] = s / L[i][i];
    }
    SFE_ICP3P_UNROLL
    for (int i = 3; i >= 0; --i) {
        double s = y[i];
        SFE_ICP3P_UNROLL
        for (int k = i + 1; k < 4; ++k)
            s -= L[k][i] * x[k];
        x[i] = s / L[i][i];
    }
    return 0;
}

// The rotation by gamma about the z axis (row-major), libpointmatcher's AngleAxis(gamma, UnitZ): no small-angle form; the
// third row and column are exact, and gamma == 0 gives the identity to the bit (cos 0 = 1, sin 0 = 0).
SFE_ICP3P_HD void icp3p_rot_z(double gamma, double *R)
{
    const double c = cos(gamma), s = sin(gamma);
    R[0] = c;
    R[1] = -s;
    R[2] = 0.0;
    R[3] = s;
    R[4] = c;
    R[5] = 0.0;
    R[6] = 0.0;
    R[7] = 0.0;
    R[8] = 1.0;
}

// PointToPlaneErrorMinimizer {force4DOF: 1} from the 15 fp64 sums over the kept pairs, F = ((p x n)_z, n) (acc[0] = W > 0,
// acc[1 .. 10] = A's upper triangle, acc[11 .. 14] = b): x = A^-1 b, R = the rotation by x[0] about z, t = x[1 .. 3].
// -> 0, or 1 where A counts as singular.
SFE_ICP3P_HD int icp3p_solve4(const double *acc, double *R, double *t)
{
    double x[4];
    if (icp3p_chol4(acc + 1, acc + 11, x))
        return 1;
    icp3p_rot_z(x[0], R);
    t[0] = x[1];
    t[1] = x[2];
    t[2] = x[3];
    return 0;
}

// PointToPlaneErrorMinimizer {force2D: 0} from the 28 fp64 sums over the kept pairs (acc[0] = W > 0, acc[1 .. 21] = A's upper
// triangle, acc[22 .. 27] = b): x = A^-1 b, R = Rodrigues(x[0 .. 2]), t = x[3 .. 5].  -> 0, or 1 where A counts as singular.
SFE_ICP3P_HD int icp3p_solve(const double *acc, double *R, double *t)
{
    double x[6];
    if (icp3p_chol6(acc + 1, acc + 22, x))
        return 1;
    icp3p_rodrigues(x, R);
    t[0] = x[3];
    t[1] = x[4];
    t[2] = x[5];
    return 0;
}
