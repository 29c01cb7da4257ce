// Stand-alone check of the transposed wave reduction's plan (sonar_slam_amd/csrc/sfe_wave_sum_plan.h), run on the CPU: the
// plan is executed on 64 simulated lanes of doubles, the way wave_sum_n (sfe_icp_common.h) executes it on the device -- DPP
// moves with the plan's controls and bank masks, the two half-wave swaps, the row totals left to right -- and every
// accumulator's total is compared, bit for bit, with a literal restatement of wave_sum (four row_shr steps with 0.0 where
// a lane has no source, then lanes 15, 31, 47, 63 added left to right).  tests/test_wave_sum_plan_host.py builds it plainly;
// under the sanitizers it is a program of its own (no GPU, nothing preloaded):
//   g++ -std=c++17 -O1 -g -Wall -Wextra -Werror -fsanitize=address,undefined -fno-sanitize-recover=all
//       tests/host/wave_sum_plan_check.cpp -o wave_sum_plan_check && ./wave_sum_plan_check
//
// What it asserts:
//   * the structure: every DPP control reaches the plan's partner in every lane that is written, every lane is written
//     by exactly one of the two masked moves of levels 2 and 3, the register j of lane l holds accumulator wsp_slot, the
//     lanes keep what wsp_keeps_upper says, wsp_final_slot / wsp_holder agree with the run, the swaps leave row r's total
//     in the r-th operand of the final chain in all 64 lanes;
//   * the sums, all nine accumulators in all 64 lanes, on: random values; values spread over 30 binades with heavy
//     cancellation; signed zeros; single non-zero lanes at 0, 15, 16, 31, 47, 63; one row alone non-zero;
//   * that the cancelling inputs can tell trees apart: (r0+r1)+(r2+r3) over the rows, and a butterfly that starts with
//     distance 8, both differ from wave_sum on them.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "../../sonar_slam_amd/csrc/sfe_wave_sum_plan.h"

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            std::fprintf(stderr, "wave_sum_plan_check: %s fails (line %d)\n", #cond, __LINE__);  \
            std::exit(1);                                                                        \
        }                                                                                        \
    } while (0)

constexpr int NL = 64, NACC = WSP_N + 1;
struct Wave {
    double v[NL];
};

static uint64_t bits(double x)
{
    uint64_t u;
    std::memcpy(&u, &x, 8);
    return u;
}

// ---- wave_sum, restated: dpp_row_shr_add<1, 2, 4, 8>, then the four row totals left to right ----
static double ref_wave_sum(const Wave &in, int row_assoc = 0)
{
    Wave v = in;
    for (int shr = 1; shr <= 8; shr *= 2) {
        Wave n;
        for (int l = 0; l < NL; ++l)
            n.v[l] = v.v[l] + ((l & 15) >= shr ? v.v[l - shr] : 0.0);
        v = n;
    }
    if (row_assoc == 1) // the wrong association, for the discrimination check only
        return (v.v[15] + v.v[31]) + (v.v[47] + v.v[63]);
    double s = v.v[15];
    s += v.v[31];
    s += v.v[47];
    s += v.v[63];
    return s;
}
// a butterfly that starts with distance 8 (another tree), rows left to right
static double wrong_butterfly(const Wave &in)
{
    Wave v = in;
    for (int d = 8; d >= 1; d /= 2) {
        Wave n;
        for (int l = 0; l < NL; ++l)
            n.v[l] = v.v[l] + v.v[l ^ d];
        v = n;
    }
    return ((v.v[0] + v.v[16]) + v.v[32]) + v.v[48];
}

// ---- the device's moves ----
static Wave dpp_mov(const Wave &old, const Wave &src, int ctrl, int banks, int level /* -1: any source lane will do */)
{
    Wave r = old;
    for (int l = 0; l < NL; ++l) {
        const int s = wsp_dpp_src(ctrl, l & 15);
        if (!wsp_bank_on(banks, l & 15))
            continue;
        CHECK(s >= 0 && s < 16); // a written lane has a source (bound_ctrl never decides a value)
        if (level >= 0)
            CHECK(s == wsp_partner(level, l & 15));
        r.v[l] = src.v[(l & ~15) | s];
    }
    return r;
}
static Wave add(const Wave &a, const Wave &b)
{
    Wave r;
    for (int l = 0; l < NL; ++l)
        r.v[l] = a.v[l] + b.v[l];
    return r;
}
static Wave trade_sel(int level, int ctrl, const Wave &lo_slot, const Wave &hi_slot)
{
    Wave keep, give;
    for (int l = 0; l < NL; ++l) {
        const bool up = (wsp_upper_mask(level) >> l) & 1;
        CHECK(up == wsp_keeps_upper(level, l & 15));
        keep.v[l] = up ? hi_slot.v[l] : lo_slot.v[l];
        give.v[l] = up ? lo_slot.v[l] : hi_slot.v[l];
    }
    return add(keep, dpp_mov(give, give, ctrl, 0xf, level));
}
template <typename F>
static void swap_pair(F src_of, const Wave &a, const Wave &b, Wave &na, Wave &nb)
{
    for (int l = 0; l < NL; ++l) {
        const int sa = src_of(0, l), sb = src_of(1, l);
        na.v[l] = sa < 64 ? a.v[sa] : b.v[sa - 64];
        nb.v[l] = sb < 64 ? a.v[sb] : b.v[sb - 64];
    }
}

// wave_sum_n: out.v[l] = the total that lane l ends up with (of accumulator wsp_final_slot(l & 15))
static Wave plan_wave_sum(const Wave (&a)[NACC])
{
    Wave b[4], c[2];
    for (int j = 0; j < 4; ++j)
        b[j] = trade_sel(0, WSP_DPP_QUAD_1032, a[j], a[j + 4]);
    Wave x = add(a[WSP_RIDER], dpp_mov(a[WSP_RIDER], a[WSP_RIDER], WSP_DPP_QUAD_1032, 0xf, 0));
    for (int j = 0; j < 2; ++j)
        c[j] = trade_sel(1, WSP_DPP_QUAD_2301, b[j], b[j + 2]);
    x = add(x, dpp_mov(x, x, WSP_DPP_QUAD_2301, 0xf, 1));
    const Wave u2 = dpp_mov(c[1], c[0], WSP_DPP_ROW_SHL4, WSP_BANKS_BIT2_CLEAR, 2);
    const Wave w2 = dpp_mov(c[0], c[1], WSP_DPP_ROW_SHR4, WSP_BANKS_BIT2_SET, 2);
    const Wave d = add(u2, w2);
    x = add(x, dpp_mov(x, x, WSP_DPP_ROW_HALF_MIRROR, 0xf, -1));
    const Wave u3 = dpp_mov(x, d, WSP_DPP_ROW_ROR8, WSP_BANKS_BIT3_CLEAR, 3);
    const Wave w3 = dpp_mov(d, x, WSP_DPP_ROW_ROR8, WSP_BANKS_BIT3_SET, 3);
    const Wave e = add(u3, w3);
    Wave p, q, r0, r1, r2, r3;
    swap_pair(wsp_swap32, e, e, p, q);
    swap_pair(wsp_swap16, p, p, r0, r1);
    swap_pair(wsp_swap16, q, q, r2, r3);
    const int order[4] = WSP_ROW_ORDER;
    const Wave *rows[4] = {&r0, &r1, &r2, &r3};
    for (int l = 0; l < NL; ++l)
        for (int k = 0; k < 4; ++k) // operand k of the chain is the total of row order[k], in every lane
            CHECK(bits(rows[k]->v[l]) == bits(e.v[16 * order[k] + (l & 15)]));
    Wave s = r0;
    s = add(s, r1);
    s = add(s, r2);
    s = add(s, r3);
    return s;
}

// ---- the structure, by the plan's own rules (no DPP): which accumulator of which lanes a lane's register sums ----
static void check_structure()
{
    // sets of lanes as 16-bit masks: reg[l][j] = (accumulator, lanes summed)
    struct Reg {
        int acc;
        unsigned lanes;
    };
    Reg cur[16][WSP_N], rider[16];
    for (int l = 0; l < 16; ++l) {
        for (int j = 0; j < WSP_N; ++j)
            cur[l][j] = {j, 1u << l};
        rider[l] = {WSP_RIDER, 1u << l};
    }
    for (int level = 0; level < 3; ++level) {
        const int n = wsp_live(level), h = n / 2;
        CHECK(wsp_live(level + 1) == (level < 2 ? h : 1));
        Reg nxt[16][WSP_N] = {};
        for (int l = 0; l < 16; ++l) {
            const int p = wsp_partner(level, l), up = wsp_keeps_upper(level, l);
            CHECK(p >= 0 && p < 16 && wsp_partner(level, p) == l && wsp_keeps_upper(level, p) != up);
            for (int j = 0; j < h; ++j) {
                const Reg mine = cur[l][j + up * h], theirs = cur[p][j + up * h];
                CHECK(mine.acc == theirs.acc && mine.acc == wsp_slot(level, l, j + up * h) && !(mine.lanes & theirs.lanes));
                nxt[l][j] = {mine.acc, mine.lanes | theirs.lanes};
                CHECK(wsp_slot(level + 1, l, j) == mine.acc);
            }
        }
        Reg nr[16];
        for (int l = 0; l < 16; ++l)
            nr[l] = {WSP_RIDER, rider[l].lanes | rider[wsp_partner(level, l)].lanes};
        std::memcpy(cur, nxt, sizeof cur);
        std::memcpy(rider, nr, sizeof rider);
    }
    int seen[NACC] = {0};
    for (int l = 0; l < 16; ++l) { // level 3: the slot against the rider
        const int p = wsp_partner(3, l);
        const Reg mine = wsp_keeps_upper(3, l) ? rider[l] : cur[l][0], theirs = wsp_keeps_upper(3, l) ? rider[p] : cur[p][0];
        CHECK(mine.acc == theirs.acc && (mine.lanes | theirs.lanes) == 0xFFFFu && !(mine.lanes & theirs.lanes));
        CHECK(mine.acc == wsp_final_slot(l));
        ++seen[mine.acc];
    }
    for (int k = 0; k < NACC; ++k) {
        CHECK(seen[k] >= 1 && wsp_holder(k) >= 0 && wsp_holder(k) < 16 && wsp_final_slot(wsp_holder(k)) == k);
        CHECK(wsp_holder(k) == k || k < WSP_N); // the rider's first holder is lane 8 = WSP_N
    }
    // the masked moves: every lane is written by exactly one of each pair
    for (int l = 0; l < 16; ++l) {
        CHECK(wsp_bank_on(WSP_BANKS_BIT2_CLEAR, l) == !((l >> 2) & 1) && wsp_bank_on(WSP_BANKS_BIT2_SET, l) == ((l >> 2) & 1));
        CHECK(wsp_bank_on(WSP_BANKS_BIT3_CLEAR, l) == !((l >> 3) & 1) && wsp_bank_on(WSP_BANKS_BIT3_SET, l) == ((l >> 3) & 1));
        CHECK(wsp_keeps_upper(2, l) == wsp_bank_on(WSP_BANKS_BIT2_SET, l) && wsp_keeps_upper(3, l) == wsp_bank_on(WSP_BANKS_BIT3_SET, l));
        const int hm = wsp_dpp_src(WSP_DPP_ROW_HALF_MIRROR, l); // the rider at level 2: any lane of the other quad of the half row
        CHECK((hm >> 3) == (l >> 3) && ((hm >> 2) & 1) != ((l >> 2) & 1));
    }
}

static long g_cases = 0;
// all nine accumulators in all 64 lanes against wave_sum
static void check_sums(const Wave (&a)[NACC])
{
    const Wave got = plan_wave_sum(a);
    for (int k = 0; k < NACC; ++k) {
        const double want = ref_wave_sum(a[k]);
        for (int l = 0; l < NL; ++l)
            if (wsp_final_slot(l & 15) == k && bits(got.v[l]) != bits(want)) {
                std::fprintf(stderr, "wave_sum_plan_check: accumulator %d lane %d: %a, wave_sum gives %a (case %ld)\n", k, l,
                             got.v[l], want, g_cases);
                std::exit(1);
            }
    }
    ++g_cases;
}

int main()
{
    check_structure();
    std::mt19937_64 rng(20240611);
    std::uniform_real_distribution<double> uni(-1.0, 1.0);
    Wave a[NACC];
    // random values
    for (int t = 0; t < 2000; ++t) {
        for (auto &w : a)
            for (double &x : w.v)
                x = uni(rng) * 1e3;
        check_sums(a);
    }
    // 30 binades, heavy cancellation: pairs of nearly opposite values at random places, plus small ones
    long diff_assoc = 0, diff_bfly = 0, n_cancel = 0;
    for (int t = 0; t < 2000; ++t) {
        for (auto &w : a) {
            for (double &x : w.v)
                x = std::ldexp(uni(rng), (int)(rng() % 30) - 10);
            for (int p = 0; p < 24; ++p) {
                const int i = (int)(rng() % NL), j = (int)(rng() % NL);
                if (i == j)
                    continue;
                const double big = std::ldexp(1.0 + 0.5 * uni(rng), 19 - (int)(rng() % 6));
                w.v[i] = big;
                w.v[j] = -big * (1.0 + std::ldexp(uni(rng), -40));
            }
        }
        check_sums(a);
        for (const auto &w : a) {
            ++n_cancel;
            diff_assoc += bits(ref_wave_sum(w, 1)) != bits(ref_wave_sum(w));
            diff_bfly += bits(wrong_butterfly(w)) != bits(ref_wave_sum(w));
        }
    }
    // the inputs tell trees apart: most of them, not a stray one
    CHECK(diff_assoc * 4 > n_cancel && diff_bfly * 4 > n_cancel);
    // signed zeros: all -0.0, all +0.0, mixed, and a lone -0.0 among +0.0 and the reverse
    for (int t = 0; t < 200; ++t) {
        for (auto &w : a)
            for (double &x : w.v)
                x = t == 0 ? -0.0 : t == 1 ? 0.0 : ((rng() & 1) ? -0.0 : 0.0);
        check_sums(a);
    }
    for (int l = 0; l < NL; ++l)
        for (int sgn = 0; sgn < 2; ++sgn) {
            for (auto &w : a)
                for (double &x : w.v)
                    x = sgn ? 0.0 : -0.0;
            for (auto &w : a)
                w.v[l] = sgn ? -0.0 : 0.0;
            check_sums(a);
        }
    // single non-zero lanes
    const int singles[6] = {0, 15, 16, 31, 47, 63};
    for (int l : singles)
        for (int t = 0; t < 20; ++t) {
            for (auto &w : a) {
                for (double &x : w.v)
                    x = 0.0;
                w.v[l] = uni(rng) * 1e6;
            }
            check_sums(a);
        }
    // one row alone non-zero
    for (int row = 0; row < 4; ++row)
        for (int t = 0; t < 50; ++t) {
            for (auto &w : a) {
                for (double &x : w.v)
                    x = 0.0;
                for (int l = 0; l < 16; ++l)
                    w.v[16 * row + l] = std::ldexp(uni(rng), (int)(rng() % 30) - 10);
            }
            check_sums(a);
        }
    std::printf("wave_sum_plan_check: ok (%ld cases; of %ld cancelling inputs %ld tell the row association apart, %ld the butterfly)\n",
                g_cases, n_cancel, diff_assoc, diff_bfly);
    return 0;
}
