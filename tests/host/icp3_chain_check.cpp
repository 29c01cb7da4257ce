// CPU check of sonar_slam_amd/csrc/sfe_icp3_chain.h: the data-point stage predicates, the outlier filters' keep test, the
// Bound checker's test and the stage-list validation of a 3-D ICP chain, evaluated on the inputs a file lists and printed,
// one line per input line, for tests/test_icp3_chain_host.py to compare with its numpy restatement bit for bit.  Floats
// travel as C99 hex literals (inf / nan by name).  Stand-alone: builds with any C++17 compiler, plain or with
// -fsanitize=address,undefined.
//
//   P kind dim remove_inside f0 f1 f2 f3 f4 f5 x y z     ->  P <keep 0|1>
//   N x y z                                              ->  N <norm as 8 hex digits>
//   O use_min min_dist use_median factor median d        ->  O <keep 0|1> <min2 bits> <med_limit bits>
//   M n                                                  ->  M <median rank>
//   B max_rot max_trans t0 .. t15                        ->  B <out 0|1> <rotation %a> <translation %a>
//   V n {kind dim f0} x n                                ->  V <code> <bad stage>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../sonar_slam_amd/csrc/sfe_icp3_chain.h"

static uint32_t bits(float v)
{
    uint32_t u;
    memcpy(&u, &v, sizeof u);
    return u;
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: icp3_chain_check <input file>\n");
        return 2;
    }
    FILE *fh = fopen(argv[1], "r");
    if (!fh) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    char line[4096];
    long n_lines = 0;
    while (fgets(line, sizeof line, fh)) {
        std::vector<std::string> tok;
        for (char *t = strtok(line, " \t\r\n"); t; t = strtok(nullptr, " \t\r\n"))
            tok.emplace_back(t);
        if (tok.empty())
            continue;
        ++n_lines;
        auto F = [&](size_t i) { return strtof(tok.at(i).c_str(), nullptr); };
        auto I = [&](size_t i) { return (int)strtol(tok.at(i).c_str(), nullptr, 10); };
        const char what = tok[0][0];
        if (what == 'P' && tok.size() == 13) {
            sfe_icp_dpf s{};
            s.kind = I(1);
            s.dim = I(2);
            s.remove_inside = I(3);
            for (int k = 0; k < 6; ++k)
                s.f[k] = F(4 + (size_t)k);
            printf("P %d\n", icp3_dpf_keep(s, F(10), F(11), F(12)) ? 1 : 0);
        } else if (what == 'N' && tok.size() == 4) {
            printf("N %08x\n", bits(icp3_dpf_norm(F(1), F(2), F(3))));
        } else if (what == 'O' && tok.size() == 7) {
            sfe_icp_outliers o{};
            o.use_min_dist = I(1);
            o.min_dist = F(2);
            o.use_median = I(3);
            o.median_factor = F(4);
            const float min2 = icp3c_mul(o.min_dist, o.min_dist), lim = icp3c_mul(o.median_factor, F(5));
            printf("O %d %08x %08x\n", icp3_ox_keep(o, min2, lim, F(6)) ? 1 : 0, bits(min2), bits(lim));
        } else if (what == 'M' && tok.size() == 2) {
            printf("M %u\n", icp3_median_rank((unsigned)strtoul(tok[1].c_str(), nullptr, 10)));
        } else if (what == 'B' && tok.size() == 19) {
            sfe_icp_outliers o{};
            o.use_bound = 1;
            o.max_rotation_norm = F(1);
            o.max_translation_norm = F(2);
            float T[16];
            for (int k = 0; k < 16; ++k)
                T[k] = F(3 + (size_t)k);
            printf("B %d %a %a\n", icp3_bound_out(o, T) ? 1 : 0, icp3_bound_rot(T), icp3_bound_trans(T));
        } else if (what == 'V' && tok.size() >= 2 && tok.size() == 2 + 3 * (size_t)(I(1) < 0 ? 0 : I(1))) {
            const int n = I(1);
            std::vector<sfe_icp_dpf> st((size_t)(n < 0 ? 0 : n));
            for (size_t k = 0; k < st.size(); ++k) {
                st[k] = sfe_icp_dpf{};
                st[k].kind = I(2 + 3 * k);
                st[k].dim = I(3 + 3 * k);
                st[k].f[0] = F(4 + 3 * k);
            }
            int bad = -1;
            const int code = icp3_dpf_validate(st.empty() ? nullptr : st.data(), n, &bad);
            printf("V %d %d\n", code, bad);
        } else {
            fprintf(stderr, "icp3_chain_check: cannot parse line %ld\n", n_lines);
            fclose(fh);
            return 1;
        }
    }
    fclose(fh);
    printf("icp3_chain_check: ok (%ld lines)\n", n_lines);
    return 0;
}
