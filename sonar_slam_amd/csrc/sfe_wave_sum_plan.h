// The plan of wave_sum_n (sfe_icp_common.h): the sums of WSP_N + 1 independent fp64 accumulators over the 64 lanes of a
// wave, all at once, in the very order of wave_sum -- inside a row of 16 lanes the balanced pairwise tree that lane 15 of
// wave_sum computes, ((v15+v14)+(v13+v12)) + ((v11+v10)+(v9+v8)) and so on, then the four row totals left to right,
// ((r0+r1)+r2)+r3.  wave_sum runs that tree once per accumulator in every lane; here the tree is transposed: at every
// level a lane and its partner split the live accumulators between them, each adds only its half, and the number of live
// values per lane halves (8 -> 4 -> 2 -> 1).  IEEE addition is commutative, so which lane of a pair performs an add does not
// change its bits (NaN payloads aside).
//
// Plain integer rules without a HIP call, shared by the device code (which takes its DPP controls, bank masks and the
// final lane -> accumulator map from here) and by tests/host/wave_sum_plan_check.cpp, which runs the plan on 64
// simulated lanes against a literal restatement of wave_sum.
//
// Level L = 0 .. 3 pairs lane l with lane l ^ (1 << L) of the same row.
//   * Levels 0 .. 2 trade the accumulators 0 .. 7 ("slots"): a lane holds n = 8 >> L live registers; with
//     b = bit L of its lane number it keeps registers [b * n/2, b * n/2 + n/2), hands the other half to its partner, and
//     register j of the next level is its kept register j + b * n/2 plus the partner's register of the same index.
//   * The ninth accumulator (the "rider") is summed the plain way on levels 0 .. 2 (every lane adds its partner's value),
//     so after level 2 every lane of a half row holds the half row's sum.
//   * Level 3 trades the one live slot against the rider: lanes 0 .. 7 of a row keep the slot, lanes 8 .. 15 the rider.
// After level 3 lane l of a row holds the row total of accumulator wsp_final_slot(l).
// The rows: every lane fetches the totals of the four rows of its accumulator (two half-wave swaps, wsp_swap32 / wsp_swap16)
// and adds them in the order WSP_ROW_ORDER, ((r0+r1)+r2)+r3.
#pragma once

#if defined(__HIPCC__)
#define SFE_WSP_HD __host__ __device__
#else
#define SFE_WSP_HD
#endif

#define WSP_N 8      // traded accumulators
#define WSP_RIDER 8  // index of the ninth
#define WSP_LEVELS 4 // log2 of a row of 16 lanes

// DPP controls of v_mov_b32 (gfx9 encoding)
#define WSP_DPP_QUAD_1032 0xB1     // quad_perm:[1,0,3,2]: lane ^ 1
#define WSP_DPP_QUAD_2301 0x4E     // quad_perm:[2,3,0,1]: lane ^ 2
#define WSP_DPP_ROW_SHL4 0x104     // lane + 4 (lanes 0-3, 8-11 of a row read their partner lane ^ 4)
#define WSP_DPP_ROW_SHR4 0x114     // lane - 4 (lanes 4-7, 12-15)
#define WSP_DPP_ROW_HALF_MIRROR 0x141 // 7 - lane inside a half row: some lane of the other quad (the rider, level 2)
#define WSP_DPP_ROW_ROR8 0x128     // lane ^ 8
// bank masks (bit q = lanes 4q .. 4q + 3 of every row are written; the others keep `old`)
#define WSP_BANKS_BIT2_CLEAR 0x5
#define WSP_BANKS_BIT2_SET 0xA
#define WSP_BANKS_BIT3_CLEAR 0x3
#define WSP_BANKS_BIT3_SET 0xC

// the lane of its row that a lane reads under a DPP control, -1 where there is none (the lane keeps `old`)
SFE_WSP_HD constexpr int wsp_dpp_src(int ctrl, int l)
{
    return ctrl < 0x100                        ? (l & ~3) | ((ctrl >> (2 * (l & 3))) & 3)
           : (ctrl > 0x100 && ctrl <= 0x10F)   ? (l + (ctrl & 15) < 16 ? l + (ctrl & 15) : -1)
           : (ctrl > 0x110 && ctrl <= 0x11F)   ? (l - (ctrl & 15) >= 0 ? l - (ctrl & 15) : -1)
           : (ctrl > 0x120 && ctrl <= 0x12F)   ? ((l - (ctrl & 15)) & 15)
           : ctrl == 0x140                     ? 15 - l
           : ctrl == 0x141                     ? (l & 8) | (7 - (l & 7))
                                               : -1;
}
SFE_WSP_HD constexpr bool wsp_bank_on(int banks, int l) { return (banks >> ((l >> 2) & 3)) & 1; }

SFE_WSP_HD constexpr int wsp_partner(int level, int l) { return l ^ (1 << level); }
// live slot registers of a lane before level `level` (level 4: after the last)
SFE_WSP_HD constexpr int wsp_live(int level) { return level < 3 ? WSP_N >> level : 1; }
// does the lane keep the upper half of its registers at this level (level 3: the rider instead of the slot)?
SFE_WSP_HD constexpr bool wsp_keeps_upper(int level, int l) { return (l >> level) & 1; }
// the lanes of a wave that keep the upper half, as a mask (bit l = lane l)
SFE_WSP_HD constexpr unsigned long long wsp_upper_mask(int level)
{
    unsigned long long m = 0;
    for (int l = 0; l < 64; ++l)
        m |= (unsigned long long)wsp_keeps_upper(level, l & 15) << l;
    return m;
}
// the accumulator in slot register j of lane l before level `level` (0 .. 3; 3 also holds after level 3 for lanes 0 .. 7)
SFE_WSP_HD constexpr int wsp_slot(int level, int l, int j)
{
    int s = j;
    for (int k = level < 3 ? level : 3; k-- > 0;)
        s += ((l >> k) & 1) * (WSP_N >> (k + 1));
    return s;
}
// the accumulator whose row total lane l of a row holds after level 3; wsp_holder: the first lane that holds it
SFE_WSP_HD constexpr int wsp_final_slot(int l) { return (l & 8) ? WSP_RIDER : ((l & 1) << 2) | (l & 2) | ((l >> 2) & 1); }
SFE_WSP_HD constexpr int wsp_holder(int acc) { return acc == WSP_RIDER ? 8 : ((acc & 1) << 2) | (acc & 2) | ((acc >> 2) & 1); }

// The rows.  v_permlane32_swap a, b: rows 2, 3 of a change places with rows 0, 1 of b; v_permlane16_swap a, b: rows 1, 3
// of a change places with rows 0, 2 of b.  which = 0: where lane l (0 .. 63) of the new a comes from, which = 1: of the new
// b; the answer is 64 * (0 for the old a, 1 for the old b) + lane.
SFE_WSP_HD constexpr int wsp_swap32(int which, int l)
{
    return which == 0 ? (l >= 32 ? 64 + l - 32 : l) : (l < 32 ? l + 32 : 64 + l);
}
SFE_WSP_HD constexpr int wsp_swap16(int which, int l)
{
    return which == 0 ? ((l & 16) ? 64 + l - 16 : l) : ((l & 16) ? 64 + l : l + 16);
}
// With e = the register of the row totals: (a, b) = swap32(e, e), then (a0, a1) = swap16(a, a) and (b0, b1) = swap16(b, b)
// leave row 0's total in a0, row 1's in a1, row 2's in b0 and row 3's in b1, in every lane of the four rows; the total is
// ((a0 + a1) + b0) + b1.
#define WSP_ROW_ORDER {0, 1, 2, 3}

static_assert(wsp_dpp_src(WSP_DPP_QUAD_1032, 6) == 7 && wsp_dpp_src(WSP_DPP_QUAD_2301, 13) == 15, "quad_perm encoding");
static_assert(wsp_dpp_src(WSP_DPP_ROW_SHL4, 9) == 13 && wsp_dpp_src(WSP_DPP_ROW_SHR4, 3) == -1, "row shifts");
static_assert(wsp_dpp_src(WSP_DPP_ROW_ROR8, 3) == 11 && wsp_dpp_src(WSP_DPP_ROW_HALF_MIRROR, 9) == 14, "row_ror, half mirror");
static_assert(wsp_final_slot(wsp_holder(6)) == 6 && wsp_final_slot(wsp_holder(WSP_RIDER)) == WSP_RIDER, "holders");
static_assert(wsp_slot(3, 5, 0) == wsp_final_slot(5) && wsp_slot(1, 3, 2) == 6, "slots");
