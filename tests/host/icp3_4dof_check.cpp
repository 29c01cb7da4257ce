// The one-lane arithmetic of the 4-DoF point-to-plane step of the 3-D ICP (sonar_slam_amd/csrc/sfe_icp3_plane.h:
// icp3p_chol4, icp3p_rot_z, icp3p_solve4) on the CPU, for tests/test_icp3_4dof_host.py, which holds what this program
// prints against numpy.
//
//   g++ -std=c++17 -O1 -Wall -Wextra -Werror tests/host/icp3_4dof_check.cpp -o icp3_4dof_check
//   (the test builds it a second time with -g -fsanitize=address,undefined -fno-sanitize-recover=all)
//
// Standard input, one request per line, answered by one line of %.17g numbers:
//   A a00 a01 .. a33 b0 .. b3 -> icp3p_chol4 on the upper triangle (10 entries, row by row) and b: the singular flag, then x (4
//                                entries, zeros where singular)
//   Z gamma                   -> the 9 entries of icp3p_rot_z(gamma)
//   S acc0 .. acc14           -> icp3p_solve4: the singular flag, R (9) and t (3) (zeros where singular)
// Without input it only runs the checks below and prints "icp3_4dof_check: ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "../../sonar_slam_amd/csrc/sfe_icp3_plane.h"

static_assert(ICP3P4_NSUM == 1 + 10 + 4, "W, the upper triangle of the 4 x 4 matrix, b");

static int failures = 0;

static void expect(bool ok, const char *what)
{
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        ++failures;
    }
}

static void self_checks()
{
    // the solve: non-finite and zero systems count as singular and leave x alone
    double A[10], b[4] = {1, 2, 3, 4}, x[4] = {7, 7, 7, 7};
    for (double fill : {0.0, (double)NAN, (double)INFINITY, -(double)INFINITY}) {
        for (int i = 0; i < 10; ++i)
            A[i] = fill;
        expect(icp3p_chol4(A, b, x) == 1 && x[0] == 7 && x[3] == 7, "a zero or non-finite A is singular and leaves x alone");
    }
    // the identity system gives b
    const double I4[10] = {1, 0, 0, 0, 1, 0, 0, 1, 0, 1};
    expect(icp3p_chol4(I4, b, x) == 0 && x[0] == 1 && x[1] == 2 && x[2] == 3 && x[3] == 4, "A = I gives x = b");
    // a zero diagonal entry behind the first: pivot 0 is not above 1e-10 x 0
    const double noz[10] = {2, 0, 0, 0, 3, 0, 0, 4, 0, 0};
    expect(icp3p_chol4(noz, b, x) == 1, "A33 = 0 is singular");
    const double noyaw[10] = {0, 0, 0, 0, 3, 0, 0, 4, 0, 5};
    expect(icp3p_chol4(noyaw, b, x) == 1, "A00 = 0 is singular");
    // the rotation about z: the identity at zero to the bit; the third row and column exact everywhere
    double R[9];
    icp3p_rot_z(0.0, R);
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int i = 0; i < 9; ++i)
        expect(R[i] == I[i], "gamma = 0 gives the identity");
    for (double g : {-3.0, -1e-9, 1e-300, 0.7, 2.5, 1e6}) {
        icp3p_rot_z(g, R);
        expect(R[2] == 0.0 && R[5] == 0.0 && R[6] == 0.0 && R[7] == 0.0 && R[8] == 1.0, "the z row and column are exact");
        expect(R[0] == R[4] && R[1] == -R[3], "[[c, -s], [s, c]]");
        expect(std::fabs(R[0] * R[0] + R[3] * R[3] - 1.0) < 1e-15, "unit columns");
    }
    icp3p_rot_z(NAN, R); // (no crash; the result is not finite and the checkers report it)
    expect(!std::isfinite(R[0]) && R[8] == 1.0, "a NaN angle does not pass for a rotation");
    // the whole step on a singular system reports it
    double acc[ICP3P4_NSUM], t[3];
    for (int i = 0; i < ICP3P4_NSUM; ++i)
        acc[i] = 0.0;
    expect(icp3p_solve4(acc, R, t) == 1, "zero sums are singular");
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
        double v[ICP3P4_NSUM];
        const int want = kind == "A" ? 14 : kind == "Z" ? 1 : kind == "S" ? ICP3P4_NSUM : -1;
        int n = 0;
        std::string tok;
        while (n < want && (in >> tok)) // (strtod, not operator>>: it reads "nan" and "inf")
            v[n++] = std::strtod(tok.c_str(), nullptr);
        if (want < 0 || n != want) {
            std::printf("FAILED: bad request line: %s\n", line.c_str());
            ++failures;
            continue;
        }
        if (kind == "A") {
            double o[5] = {0, 0, 0, 0, 0};
            o[0] = icp3p_chol4(v, v + 10, o + 1);
            print_line(o, 5);
        } else if (kind == "Z") {
            double R[9];
            icp3p_rot_z(v[0], R);
            print_line(R, 9);
        } else {
            double o[13] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            o[0] = icp3p_solve4(v, o + 1, o + 10);
            print_line(o, 13);
        }
    }
    if (failures)
        return 1;
    std::printf("icp3_4dof_check: ok\n");
    return 0;
}
