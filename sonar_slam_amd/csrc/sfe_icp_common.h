// Device helpers shared by the ICP kernels (sfe_icp.hip: brute-force tile scan, sfe_icp_sweep.hip:
// strip-sweep search).  Every float expression that decides a match or a weight is written with
// explicit IEEE roundings (no contraction) so both kernels and the oracle take the same decisions.
#pragma once
#include "sfe_internal.h"
#include "sfe_icp_outlier_rules.h" // icp_median_rank, icp_ox_keep
#include "sfe_wave_sum_plan.h"

#ifndef ICP_THREADS
#define ICP_THREADS 1024
#endif
#define ICP_WAVES (ICP_THREADS / 64)
#define ICP_TCAP 8192 // target points resident in LDS (64 KiB as float2)
#define ICP_PB 8      // max source points per lane per pass over the target
#define ICP_CH 16     // target points per chunk of the two-level arg-min
#define ICP_KMAX 16   // max neighbours for the PCA normals
#define ICP_MAX_HIST 64 // transformation history kept for the differential checker
#define ICP_PIVOT_RTOL 1e-10 // Cholesky pivot / diagonal entry below which the point-to-plane system counts as singular

struct IcpJob {
    int src_start, n_src, tgt_start, n_tgt;
    long long scratch_off; // offset (in points) of this job's slice of the NN scratch
    long long nrm_off;     // offset (in points) of this job's slice of the normals scratch
};

__device__ __forceinline__ float f_mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float f_add(float a, float b) { return __fadd_rn(a, b); }

// x' = (a*x + b*y) + c with every product/sum rounded to float (Eigen's coefficient product)
__device__ __forceinline__ float affine1(float a, float b, float c, float x, float y)
{
    return f_add(f_add(f_mul(a, x), f_mul(b, y)), c);
}

// v + (v of the lane `SHR` places to the left in the same row of 16 lanes, 0.0 where there is none): DPP
// row_shr, no address register and no LDS crossbar (the __shfl form kept six loop-invariant address
// VGPRs alive, which the 64-VGPR ICP kernels spilled and re-loaded around every reduction)
template <int SHR>
__device__ __forceinline__ double dpp_row_shr_add(double v)
{
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const int lo2 = __builtin_amdgcn_update_dpp(0, lo, 0x110 + SHR, 0xf, 0xf, false);
    const int hi2 = __builtin_amdgcn_update_dpp(0, hi, 0x110 + SHR, 0xf, 0xf, false);
    return v + __hiloint2double(hi2, lo2);
}

// sum over the 64 lanes, same value in every lane; fixed order (deterministic): inclusive scan inside
// each row of 16 lanes, then the four row totals left to right
__device__ __forceinline__ double wave_sum(double v)
{
    v = dpp_row_shr_add<1>(v);
    v = dpp_row_shr_add<2>(v);
    v = dpp_row_shr_add<4>(v);
    v = dpp_row_shr_add<8>(v);
    const int lo = __double2loint(v), hi = __double2hiint(v);
    double s = __hiloint2double(__builtin_amdgcn_readlane(hi, 15), __builtin_amdgcn_readlane(lo, 15));
    s += __hiloint2double(__builtin_amdgcn_readlane(hi, 31), __builtin_amdgcn_readlane(lo, 31));
    s += __hiloint2double(__builtin_amdgcn_readlane(hi, 47), __builtin_amdgcn_readlane(lo, 47));
    s += __hiloint2double(__builtin_amdgcn_readlane(hi, 63), __builtin_amdgcn_readlane(lo, 63));
    return s;
}

// v of the lane that the DPP control names (sfe_wave_sum_plan.h); the lanes outside `BANKS` keep `old`.  (With every bank
// written and a control under which every lane has a source, `old` is never read: bound_ctrl says so, which spares the
// copy of `old` into the destination.)
template <int CTRL, int BANKS = 0xf>
__device__ __forceinline__ double dpp_mov_f64(double old, double v)
{
    constexpr bool ALL = BANKS == 0xf;
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(v), CTRL, 0xf, BANKS, ALL);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(v), CTRL, 0xf, BANKS, ALL);
    return __hiloint2double(hi, lo);
}

// a constant lane mask as a per-lane condition, set up by two scalar moves where it is used (a compare of the lane number,
// and a literal that the compiler sees, are hoisted out of the ICP iteration loop and spilled: two v_readlane per use)
template <unsigned long long M>
__device__ __forceinline__ bool wsp_lane_mask()
{
    static_assert((unsigned)(M >> 32) == (unsigned)M, "the same word for both halves of the wave");
    unsigned m;
    asm volatile("s_mov_b32 %0, %1" : "=s"(m) : "n"((unsigned)M));
    return __builtin_amdgcn_inverse_ballot_w64(((unsigned long long)m << 32) | m);
}

// one traded register of levels 0 and 1 (a lane bit that the bank masks cannot tell apart): the lanes with `up` keep
// `hi_slot` and add their partner's, the others `lo_slot`
template <int CTRL>
__device__ __forceinline__ double wsp_trade(bool up, double lo_slot, double hi_slot)
{
    const double keep = up ? hi_slot : lo_slot, give = up ? lo_slot : hi_slot;
    return keep + dpp_mov_f64<CTRL>(0.0, give);
}

// The nine sums of wave_sum(a[0]) .. wave_sum(a[8]) at once, bit for bit (NaN payloads aside), by the transposed tree of
// sfe_wave_sum_plan.h: lane l holds the total of accumulator wsp_final_slot(l & 15) -- 11 adds per lane inside the rows (8
// for the traded accumulators, 3 for the ninth) and 3 over them instead of 63, and no per-accumulator v_readlane chain.  No address register and no LDS (see
// dpp_row_shr_add); the whole wave must be active.
__device__ __forceinline__ double wave_sum_n(const double (&a)[WSP_N + 1])
{
    static_assert(wsp_partner(0, 0) == wsp_dpp_src(WSP_DPP_QUAD_1032, 0) && wsp_partner(1, 1) == wsp_dpp_src(WSP_DPP_QUAD_2301, 1) &&
                      wsp_partner(2, 2) == wsp_dpp_src(WSP_DPP_ROW_SHL4, 2) && wsp_partner(2, 14) == wsp_dpp_src(WSP_DPP_ROW_SHR4, 14) &&
                      wsp_partner(3, 5) == wsp_dpp_src(WSP_DPP_ROW_ROR8, 5),
                  "the DPP controls reach the plan's partners (all lanes: tests/host/wave_sum_plan_check.cpp)");
    const bool up0 = wsp_lane_mask<wsp_upper_mask(0)>(), up1 = wsp_lane_mask<wsp_upper_mask(1)>();
    double b[4], c[2];
    // level 0: 8 -> 4
#pragma unroll
    for (int j = 0; j < 4; ++j)
        b[j] = wsp_trade<WSP_DPP_QUAD_1032>(up0, a[j], a[j + 4]);
    double x = a[WSP_RIDER] + dpp_mov_f64<WSP_DPP_QUAD_1032>(0.0, a[WSP_RIDER]);
    // level 1: 4 -> 2
#pragma unroll
    for (int j = 0; j < 2; ++j)
        c[j] = wsp_trade<WSP_DPP_QUAD_2301>(up1, b[j], b[j + 2]);
    x = x + dpp_mov_f64<WSP_DPP_QUAD_2301>(0.0, x);
    // level 2: 2 -> 1, told apart by the banks: u = the partner's c[0] where bit 2 is clear, the own c[1] elsewhere; w the other way round
    const double u2 = dpp_mov_f64<WSP_DPP_ROW_SHL4, WSP_BANKS_BIT2_CLEAR>(c[1], c[0]);
    const double w2 = dpp_mov_f64<WSP_DPP_ROW_SHR4, WSP_BANKS_BIT2_SET>(c[0], c[1]);
    const double d = u2 + w2;
    x = x + dpp_mov_f64<WSP_DPP_ROW_HALF_MIRROR>(0.0, x);
    // level 3: the slot against the rider
    const double u3 = dpp_mov_f64<WSP_DPP_ROW_ROR8, WSP_BANKS_BIT3_CLEAR>(x, d);
    const double w3 = dpp_mov_f64<WSP_DPP_ROW_ROR8, WSP_BANKS_BIT3_SET>(d, x);
    const double e = u3 + w3;
    // the rows: ((r0 + r1) + r2) + r3
    const unsigned lo = (unsigned)__double2loint(e), hi = (unsigned)__double2hiint(e);
    const auto l32 = __builtin_amdgcn_permlane32_swap(lo, lo, false, false), h32 = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    const auto l01 = __builtin_amdgcn_permlane16_swap(l32[0], l32[0], false, false),
               h01 = __builtin_amdgcn_permlane16_swap(h32[0], h32[0], false, false),
               l23 = __builtin_amdgcn_permlane16_swap(l32[1], l32[1], false, false),
               h23 = __builtin_amdgcn_permlane16_swap(h32[1], h32[1], false, false);
    double s = __hiloint2double((int)h01[0], (int)l01[0]);
    s += __hiloint2double((int)h01[1], (int)l01[1]);
    s += __hiloint2double((int)h23[0], (int)l23[0]);
    s += __hiloint2double((int)h23[1], (int)l23[1]);
    return s;
}

// minimum over the 64 lanes (NaN-free inputs), same value in every lane; DPP like wave_sum
template <int SHR>
__device__ __forceinline__ float dpp_row_shr_min(float v)
{
    const int o = __builtin_amdgcn_update_dpp(0x7F800000 /* +inf where there is no source lane */, __float_as_int(v),
                                              0x110 + SHR, 0xf, 0xf, false);
    return fminf(v, __int_as_float(o));
}
__device__ __forceinline__ float wave_min(float v)
{
    v = dpp_row_shr_min<1>(v);
    v = dpp_row_shr_min<2>(v);
    v = dpp_row_shr_min<4>(v);
    v = dpp_row_shr_min<8>(v);
    const int b = __float_as_int(v);
    return fminf(fminf(__int_as_float(__builtin_amdgcn_readlane(b, 15)), __int_as_float(__builtin_amdgcn_readlane(b, 31))),
                 fminf(__int_as_float(__builtin_amdgcn_readlane(b, 47)), __int_as_float(__builtin_amdgcn_readlane(b, 63))));
}

// inclusive prefix sum over the 64 lanes (unsigned), DPP inside the rows + the row totals of the rows before
template <int SHR>
__device__ __forceinline__ unsigned dpp_row_shr_addu(unsigned v)
{
    return v + (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x110 + SHR, 0xf, 0xf, false);
}
__device__ __forceinline__ unsigned wave_inclusive_scan(unsigned v)
{
    v = dpp_row_shr_addu<1>(v);
    v = dpp_row_shr_addu<2>(v);
    v = dpp_row_shr_addu<4>(v);
    v = dpp_row_shr_addu<8>(v);
    const unsigned r0 = (unsigned)__builtin_amdgcn_readlane((int)v, 15), r1 = (unsigned)__builtin_amdgcn_readlane((int)v, 31),
                   r2 = (unsigned)__builtin_amdgcn_readlane((int)v, 47);
    const int row = (threadIdx.x & 63) >> 4;
    return v + (row > 0 ? r0 : 0u) + (row > 1 ? r1 : 0u) + (row > 2 ? r2 : 0u);
}

// block-wide sum of NV doubles per thread; result valid in every thread (NTH = threads of the workgroup)
template <int NV, int NTH = ICP_THREADS>
__device__ __forceinline__ void block_sum(double (&v)[NV], double *s_red /* (NTH/64)*NV + NV */)
{
    constexpr int NWV = NTH / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const double s = wave_sum(v[i]);
        if (lane == 0)
            s_red[wave * NV + i] = s;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        double s = 0;
        for (int w = 0; w < NWV; ++w) // fixed order: deterministic
            s += s_red[w * NV + threadIdx.x];
        s_red[NWV * NV + threadIdx.x] = s;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i)
        v[i] = s_red[NWV * NV + i];
    __syncthreads();
}

__device__ __forceinline__ void mat3_mul(const float *a, const float *b, float *c)
{
    float r[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float s = f_mul(a[i * 3], b[j]);
            s = f_add(s, f_mul(a[i * 3 + 1], b[3 + j]));
            s = f_add(s, f_mul(a[i * 3 + 2], b[6 + j]));
            r[i * 3 + j] = s;
        }
#pragma unroll
    for (int i = 0; i < 9; ++i)
        c[i] = r[i];
}

__device__ __forceinline__ float dist2(float px, float py, float tx, float ty)
{
    // fl(fl(dx*dx) + fl(dy*dy)): how the oracle / libnabo accumulate the squared distance
    const float dx = f_add(px, -tx), dy = f_add(py, -ty);
    return f_add(f_mul(dx, dx), f_mul(dy, dy));
}


// Checker state of one job: the history lives in LDS and only thread 0 touches it.
struct IcpCheck {
    float *hist_c, *hist_s, *hist_x, *hist_y;
    int nhist, counter, iters;
};

// k_sel-th smallest (0-based) finite distance of nn_d2[0 .. ns) by radix select on the float bit patterns, four passes of
// eight bits over the histogram of the job's shared block (Shared: hist[256], sel_prefix, sel_k); called by the whole
// workgroup of ICP_THREADS.  The callers keep k_sel below the number nfin >= 1 of finite distances (the trimmed rank as
// min(k_sel, nfin - 1), the median's as nfin / 2), and only finite distances are stored and counted, so the bucket loop
// always breaks inside the histogram; its bound matters only to a k_sel that is not below the histogram's total.
template <class Shared>
__device__ __forceinline__ float icp_select_kth(Shared &S, const float *nn_d2, int ns, int tid, unsigned k_sel)
{
    if (tid == 0) {
        S.sel_k = k_sel;
        S.sel_prefix = 0;
    }
    __syncthreads();
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256)
            S.hist[tid] = 0;
        __syncthreads();
        const unsigned prefix = S.sel_prefix;
        const unsigned himask = (shift == 24) ? 0u : (0xFFFFFFFFu << (shift + 8));
        for (int i = tid; i < ns; i += ICP_THREADS) {
            const float d = nn_d2[i];
            if (d != INFINITY) {
                const unsigned u = __float_as_uint(d); // d >= 0: bit pattern order == value order
                if ((u & himask) == prefix)
                    atomicAdd(&S.hist[(u >> shift) & 255u], 1u);
            }
        }
        __syncthreads();
        if (tid == 0) {
            unsigned k = S.sel_k, b = 0;
            for (; b < 255; ++b) { // (b stops at 255: the shift below stays inside the word whatever the histogram holds)
                const unsigned h = S.hist[b];
                if (k < h)
                    break;
                k -= h;
            }
            S.sel_k = k;
            S.sel_prefix = prefix | (b << shift);
        }
        __syncthreads();
    }
    return __uint_as_float(S.sel_prefix);
}

// BoundTransformationChecker on T_iter: rotation acosf(T00) (NaN when |T00| > 1: never out of bounds), translation
// sqrtf(tx*tx + ty*ty) in float
__device__ __forceinline__ bool icp_bound_out(const sfe_icp_outliers &O, const float (&T)[9])
{
    const float rot = acosf(T[0]);
    const float tr = sqrtf(f_add(f_mul(T[2], T[2]), f_mul(T[5], T[5])));
    return rot > O.max_rotation_norm || tr > O.max_translation_norm;
}

// One lane: error minimiser solve (closed-form weighted Kabsch, or Cholesky of the 2-D
// point-to-plane normal equations) from the reduced sums `acc`, T_iter = T_step * T_iter, then
// the Counter / Differential transformation checkers (libpointmatcher order) and, where listed, the Bound checker in
// its place of the list (sfe_icp_outliers; OX builds only).  Ti = current T_iter (registers), Ti_lds = where the new one goes.
template <bool OX>
__device__ __forceinline__ void icp_solve_and_check(const sfe_icp_params &P, const sfe_icp_outliers &O,
                                                    const double (&acc)[10], const float (&Ti)[9], float *Ti_lds,
                                                    IcpCheck &C, int &status, int &iterate)
{
    float *hist_c = C.hist_c, *hist_s = C.hist_s, *hist_x = C.hist_x, *hist_y = C.hist_y;
    int &nhist = C.nhist, &counter = C.counter, &iters = C.iters;
    status = SFE_ICP_OK;
    iterate = 1;
    float Ts[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (acc[0] == 0.0) {
        status = SFE_ICP_NO_POINT;
    } else if (P.minimizer == 0) {
        const double W = acc[0];
        const double mpx = acc[1] / W, mpy = acc[2] / W, mqx = acc[3] / W, mqy = acc[4] / W;
        const double m00 = acc[5] - acc[3] * mpx, m01 = acc[6] - acc[3] * mpy;
        const double m10 = acc[7] - acc[4] * mpx, m11 = acc[8] - acc[4] * mpy;
        const double Sx = m00 + m11, Kx = m10 - m01;
        const double h = sqrt(Sx * Sx + Kx * Kx);
        const double c = (h == 0) ? 1.0 : Sx / h;
        const double s = (h == 0) ? 0.0 : Kx / h;
        const double tx = mqx - (c * mpx - s * mpy);
        const double ty = mqy - (s * mpx + c * mpy);
        Ts[0] = (float)c;
        Ts[1] = (float)-s;
        Ts[2] = (float)tx;
        Ts[3] = (float)s;
        Ts[4] = (float)c;
        Ts[5] = (float)ty;
    } else {
        // a pivot that has lost ten digits against its diagonal entry = rank-deficient system (in exact arithmetic the
        // pivot is zero, in floating point its sign is summation-order noise): decided by a relative test, the same
        // expression as the oracle's, so that every implementation reports such systems the same way
        const double l00 = sqrt(acc[1]);
        const double l10 = acc[2] / l00, l20 = acc[3] / l00;
        const double p11 = acc[4] - l10 * l10;
        const double l11 = sqrt(p11);
        const double l21 = (acc[5] - l20 * l10) / l11;
        const double p22 = acc[6] - l20 * l20 - l21 * l21;
        const double l22 = sqrt(p22);
        if (!(l00 > 0) || !(p11 > ICP_PIVOT_RTOL * acc[4]) || !(p22 > ICP_PIVOT_RTOL * acc[6])) {
            status = SFE_ICP_SINGULAR;
        } else {
            const double y0 = acc[7] / l00;
            const double y1 = (acc[8] - l10 * y0) / l11;
            const double y2 = (acc[9] - l20 * y0 - l21 * y1) / l22;
            const double x2 = y2 / l22;
            const double x1 = (y1 - l21 * x2) / l11;
            const double x0 = (y0 - l10 * x1 - l20 * x2) / l00;
            const double c = cos(x0), s = sin(x0);
            Ts[0] = (float)c;
            Ts[1] = (float)-s;
            Ts[2] = (float)x1;
            Ts[3] = (float)s;
            Ts[4] = (float)c;
            Ts[5] = (float)x2;
        }
    }
    if (status == SFE_ICP_OK) {
        float Tn[9];
        mat3_mul(Ts, Ti, Tn);
        for (int i = 0; i < 9; ++i)
            Ti_lds[i] = Tn[i];
        ++iters;
        ++counter;
        // Bound: not evaluated when a Counter listed before it has just reached its limit; its status ends the job at
        // once unless a Differential checker listed before it runs first (whose NaN status then wins)
        bool out = false;
        if constexpr (OX) {
            out = O.use_bound && !((O.bound_order & 1) && counter >= P.max_iter) && icp_bound_out(O, Tn);
            if (out && !(O.bound_order & 2)) {
                status = SFE_ICP_BOUND;
                return;
            }
        }
        if (counter >= P.max_iter) {
            iterate = 0; // CounterTransformationChecker: MaxNumIterationsReached
        } else if (P.use_diff_checker) {
            if (nhist < ICP_MAX_HIST) {
                hist_c[nhist] = Tn[0];
                hist_s[nhist] = Tn[3];
                hist_x[nhist] = Tn[2];
                hist_y[nhist] = Tn[5];
                ++nhist;
            } else { // keep a sliding window (only the last smooth_len+1 entries are read)
                for (int i = 1; i < ICP_MAX_HIST; ++i) {
                    hist_c[i - 1] = hist_c[i];
                    hist_s[i - 1] = hist_s[i];
                    hist_x[i - 1] = hist_x[i];
                    hist_y[i - 1] = hist_y[i];
                }
                hist_c[ICP_MAX_HIST - 1] = Tn[0];
                hist_s[ICP_MAX_HIST - 1] = Tn[3];
                hist_x[ICP_MAX_HIST - 1] = Tn[2];
                hist_y[ICP_MAX_HIST - 1] = Tn[5];
            }
            // rotations.size() > smoothLength; size counts the init entry (= iters + 1)
            if (iters + 1 > P.smooth_len) {
                double rsum = 0, tsum = 0;
                for (int i = nhist - 1; i >= nhist - P.smooth_len; --i) {
                    const double c1 = hist_c[i], s1 = hist_s[i], c0 = hist_c[i - 1], s0 = hist_s[i - 1];
                    rsum += fabs(atan2(s1 * c0 - c1 * s0, c1 * c0 + s1 * s0));
                    const double dx = (double)hist_x[i] - hist_x[i - 1];
                    const double dy = (double)hist_y[i] - hist_y[i - 1];
                    tsum += sqrt(dx * dx + dy * dy);
                }
                rsum /= P.smooth_len;
                tsum /= P.smooth_len;
                if (rsum < P.min_diff_rot && tsum < P.min_diff_trans)
                    iterate = 0;
                if (isnan(rsum))
                    status = SFE_ICP_NAN_ROT;
                else if (isnan(tsum))
                    status = SFE_ICP_NAN_TRANS;
            }
        }
        if constexpr (OX) {
            if (out && status == SFE_ICP_OK)
                status = SFE_ICP_BOUND;
        }
    }
}
