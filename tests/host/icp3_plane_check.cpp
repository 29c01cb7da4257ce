// The one-lane arithmetic of the 3-D point-to-plane ICP (sonar_slam_amd/csrc/sfe_icp3_plane.h) on the CPU, for
// tests/test_icp3_plane_host.py, which holds what this program prints against numpy.
//
//   g++ -std=c++17 -O1 -Wall -Wextra -Werror tests/host/icp3_plane_check.cpp -o icp3_plane_check
//   (the test builds it a second time with -g -fsanitize=address,undefined -fno-sanitize-recover=all)
//
// Standard input, one request per line, answered by one line of %.17g numbers:
//   C c00 c01 .. c22          -> the 3 entries of icp3p_normal(C)
//   A a00 a01 .. a55 b0 .. b5 -> icp3p_chol6 on the upper triangle (21 entries, row by row) and b: the singular flag, then x (6
//                                entries, zeros where singular)
//   R r0 r1 r2                -> the 9 entries of icp3p_rodrigues(r)
//   S acc0 .. acc27           -> icp3p_solve: the singular flag, R (9) and t (3) (zeros where singular)
// Without input it only runs the checks below and prints "icp3_plane_check: ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "../../sonar_slam_amd/csrc/sfe_icp3_plane.h"

static int failures = 0;

static void expect(bool ok, const char *what)
{
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        ++failures;
    }
}

static bool unit(const double *n, double tol)
{
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(n[i]))
            return false;
    return std::fabs(std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]) - 1.0) <= tol;
}

static void self_checks()
{
    double n[3];
    const double zero[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    icp3p_normal(zero, n);
    expect(n[0] == 1.0 && n[1] == 0.0 && n[2] == 0.0, "C = 0 gives (1, 0, 0)");
    double bad[9];
    for (int i = 0; i < 9; ++i)
        bad[i] = NAN;
    icp3p_normal(bad, n);
    expect(n[0] == 1.0 && n[1] == 0.0 && n[2] == 0.0, "NaN C gives (1, 0, 0)");
    for (int i = 0; i < 9; ++i)
        bad[i] = INFINITY;
    icp3p_normal(bad, n);
    expect(unit(n, 1e-15), "infinite C gives a finite unit vector");
    // rank 1 (collinear points along d): a unit vector across d
    const double d[3] = {0.3, -1.7, 2.2};
    double C1[9];
    for (int e = -300; e <= 300; e += 100) {
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j)
                C1[3 * i + j] = d[i] * d[j] * std::pow(10.0, e);
        icp3p_normal(C1, n);
        expect(unit(n, 1e-15), "rank-1 C gives a finite unit vector");
        expect(std::fabs(n[0] * d[0] + n[1] * d[1] + n[2] * d[2]) < 1e-14, "... across the line");
    }
    // equal eigenvalues go to the lowest column
    const double eq[9] = {2, 0, 0, 0, 2, 0, 0, 0, 5};
    icp3p_normal(eq, n);
    expect(n[0] == 1.0 && n[1] == 0.0 && n[2] == 0.0, "equal eigenvalues: the lowest column");
    // the solve: non-finite and zero systems count as singular and leave x alone
    double A[21], b[6] = {1, 2, 3, 4, 5, 6}, x[6] = {7, 7, 7, 7, 7, 7};
    for (int i = 0; i < 21; ++i)
        A[i] = 0.0;
    expect(icp3p_chol6(A, b, x) == 1 && x[0] == 7, "A = 0 is singular");
    for (int i = 0; i < 21; ++i)
        A[i] = NAN;
    expect(icp3p_chol6(A, b, x) == 1 && x[0] == 7, "NaN A is singular");
    for (int i = 0; i < 21; ++i)
        A[i] = INFINITY;
    expect(icp3p_chol6(A, b, x) == 1 && x[0] == 7, "infinite A is singular");
    // Rodrigues at zero is the identity, to the bit
    double R[9];
    const double r0[3] = {0, 0, 0};
    icp3p_rodrigues(r0, R);
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int i = 0; i < 9; ++i)
        expect(R[i] == I[i], "theta = 0 gives the identity");
    const double rn[3] = {NAN, 0, 1};
    icp3p_rodrigues(rn, R); // (no crash; the result is not finite and the checkers report it)
    expect(!std::isfinite(R[0]), "NaN in r does not pass for a rotation");
}

static void print_line(const double *v, int n)
{
    for (int i = 0; i < n; ++i)
        std::printf(i ? " %.17g" : "%.17g", v[i]);
    std::printf("\n");
}

int main()
{
    self_checks();
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind;
        if (!(in >> kind))
            continue;
        double v[ICP3P_NSUM];
        const int want = kind == "C" ? 9 : kind == "A" ? 27 : kind == "R" ? 3 : kind == "S" ? ICP3P_NSUM : -1;
        int n = 0;
        std::string tok;
        while (n < want && (in >> tok)) // (strtod, not operator>>: it reads "nan" and "inf")
            v[n++] = std::strtod(tok.c_str(), nullptr);
        if (want < 0 || n != want) {
            std::printf("FAILED: bad request line: %s\n", line.c_str());
            ++failures;
            continue;
        }
        if (kind == "C") {
            double nv[3];
            icp3p_normal(v, nv);
            print_line(nv, 3);
        } else if (kind == "A") {
            double o[7] = {0, 0, 0, 0, 0, 0, 0};
            o[0] = icp3p_chol6(v, v + 21, o + 1);
            print_line(o, 7);
        } else if (kind == "R") {
            double R[9];
            icp3p_rodrigues(v, R);
            print_line(R, 9);
        } else {
            double o[13] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            o[0] = icp3p_solve(v, o + 1, o + 10);
            print_line(o, 13);
        }
    }
    if (failures)
        return 1;
    std::printf("icp3_plane_check: ok\n");
    return 0;
}
