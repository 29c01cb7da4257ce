// The one-lane arithmetic of the 3-D ICP kernel (sonar_slam_amd/csrc/sfe_icp3_solve.h) on the CPU, for
// tests/test_icp3_ref_host.py, which holds what this program prints against numpy.
//
//   g++ -std=c++17 -O1 -Wall -Wextra -Werror tests/host/icp3_solve_check.cpp -o icp3_solve_check
//   (for whoever changes the header: add -g -fsanitize=address,undefined and run the same way)
//
// Standard input, one request per line, answered by one line of %.17g numbers:
//   H h00 h01 .. h22          -> the 9 entries of icp3_rotation(H)
//   S acc0 .. acc15           -> the 9 entries of R and the 3 of t of icp3_solve(acc)
//   Q a00 .. a22 b00 .. b22   -> icp3_rot_dist of the two blocks (rounded to float first, as the kernel holds them),
//                                then the two quaternions (w x y z each)
// Without input it only runs the checks below (degenerate H stays finite) and prints "icp3_solve_check: ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <iostream>

#include "../../sonar_slam_amd/csrc/sfe_icp3_solve.h"

static int failures = 0;

static void expect(bool ok, const char *what)
{
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        ++failures;
    }
}

static bool proper_rotation(const double *R, double tol)
{
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(R[i]))
            return false;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0;
            for (int k = 0; k < 3; ++k)
                s += R[3 * i + k] * R[3 * j + k];
            if (std::fabs(s - (i == j ? 1.0 : 0.0)) > tol)
                return false;
        }
    const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
    return std::fabs(det - 1.0) <= tol;
}

static void self_checks()
{
    double R[9];
    const double zero[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    icp3_rotation(zero, R);
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int i = 0; i < 9; ++i)
        expect(R[i] == I[i], "H = 0 gives the identity");
    // rank 1 (all pairs collinear): R is undetermined, but a finite proper rotation comes back
    const double u[3] = {0.3, -1.7, 2.2}, w[3] = {-0.9, 0.4, 1.1};
    double H1[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            H1[3 * i + j] = u[i] * w[j];
    icp3_rotation(H1, R);
    expect(proper_rotation(R, 1e-14), "rank-1 H gives a finite proper rotation");
    // tiny and huge scales
    double Hs[9];
    for (int e = -300; e <= 300; e += 100) {
        for (int i = 0; i < 9; ++i)
            Hs[i] = (I[i] + 0.1 * H1[i]) * std::pow(10.0, e);
        icp3_rotation(Hs, R);
        expect(proper_rotation(R, 1e-14), "scaled H gives a finite proper rotation");
    }
    // non-finite sums end (no endless loop) with non-finite output, and the checker's distance is NaN for a NaN block
    Hs[4] = NAN;
    icp3_rotation(Hs, R);
    expect(!proper_rotation(R, 1.0), "NaN in H does not pass for a rotation");
    float a[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, b[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    expect(icp3_rot_dist(a, b) == 0.0, "distance of the identity from itself");
    b[0] = NAN;
    expect(std::isnan(icp3_rot_dist(a, b)), "NaN block gives a NaN distance");
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
        double v[18];
        const int want = kind == "H" ? 9 : kind == "S" ? ICP3_NSUM : kind == "Q" ? 18 : -1;
        int n = 0;
        std::string tok;
        while (n < want && (in >> tok)) // (strtod, not operator>>: it reads "nan" and "inf")
            v[n++] = std::strtod(tok.c_str(), nullptr);
        if (want < 0 || n != want) {
            std::printf("FAILED: bad request line: %s\n", line.c_str());
            ++failures;
            continue;
        }
        if (kind == "H") {
            double R[9];
            icp3_rotation(v, R);
            print_line(R, 9);
        } else if (kind == "S") {
            double o[12];
            icp3_solve(v, o, o + 9);
            print_line(o, 12);
        } else {
            float a[9], b[9];
            double da[9], db[9], o[9];
            for (int i = 0; i < 9; ++i) {
                a[i] = (float)v[i];
                b[i] = (float)v[9 + i];
                da[i] = a[i];
                db[i] = b[i];
            }
            o[0] = icp3_rot_dist(a, b);
            icp3_quat(da, o + 1);
            icp3_quat(db, o + 5);
            print_line(o, 9);
        }
    }
    if (failures)
        return 1;
    std::printf("icp3_solve_check: ok\n");
    return 0;
}
