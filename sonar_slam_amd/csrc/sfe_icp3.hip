// 3-D ICP on gfx950: pcl.ICP.compute on N x 3 clouds with 4 x 4 guesses (pcl.cpp:198-212; PM::ICP is dimension-generic),
// the module set of the shipped config/icp.yaml -- KDTreeMatcher {knn 1}, MaxDist and TrimmedDist outlier filters,
// PointToPointErrorMinimizer (sfe_icp_params with minimizer 0), PointToPlaneErrorMinimizer {force2D: 0} (minimizer 2) or
// PointToPlaneErrorMinimizer {force4DOF: 1} (minimizer 3: yaw and translation only), Counter and Differential transformation
// checkers.  A chain written for N x 3 clouds adds, in the EXT build of the job kernel,
// the MinDist and MedianDist outlier filters and the Bound checker (sfe_icp_outliers; sfe_icp3_compute_jobs_chain_ext), and in
// front of the launch its data-point filters (sfe_icp3_dpf.hip).
//
// The rules (include/sonarfe.h at sfe_icp3_compute_jobs) are the 2-D chain's with one more coordinate:
//   centre the target on its mean, T0 = translate(-mean) * guess, reading = T0 * source            (once)
//   loop: cur = T_iter * reading
//         exact 1-NN of every cur point in the target, d2 = ((dx dx + dy dy) + dz dz), lowest index on ties, none beyond maxDist
//         keep = [d2 <= MaxDist^2] * [d2 <= quantile_ratio(finite d2)]
//         T_step = the rigid motion that minimises the kept pairs' squared distances (sfe_icp3_solve.h), rounded to float
//                  (minimizer 2: the step of the linearised point-to-plane system, sfe_icp3_plane.h; the target's surface
//                  normals come from normals3_kernel, which runs once per distinct target in front of the job kernel;
//                  minimizer 3: the same system restricted to (yaw, t), T_step a rotation about z and a translation)
//         T_iter = T_step * T_iter ; Counter / Differential checkers
//   result = translate(+mean) * (T_iter * T0)
//
// Mapping: as icp_job_kernel of sfe_icp.hip.  ONE workgroup of 1024 threads runs the whole ICP of one job; the centred target
// sits in LDS as three arrays (x, y, z: 48 KiB for 4096 points, padded with +inf) for all iterations, larger targets are
// streamed through the same tile; a lane owns up to two source points per pass and scans the tile in index order with a strict
// '<' (lowest index on ties); nearest distances and indices go to HBM scratch; the trimmed quantile is the radix select on the
// float bit patterns; the 16 sums (point-to-plane: 28, accumulated in two passes over the kept pairs; its 4-DoF form: 15, in
// one pass) are reduced in fp64 in a fixed order; one lane solves and runs the checkers.
// fp32 VALU + LDS broadcast reads, no MFMA.  LDS: 48 KiB tile + 2.1 KiB sums (point-to-plane: 3.7 KiB, 4-DoF: 2 KiB) + 1 KiB
// histogram + 3 KiB history = 55 KiB, so two workgroups fit the 160 KiB of a CU where the register count allows it.
#include "sfe_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <type_traits>
#include <utility>

#include "sfe_icp_common.h"
#include "sfe_points3.h"
#include "sfe_icp3_chain.h"
#include "sfe_icp3_plane.h"
#include "sfe_icp3_solve.h"

#define ICP3_TCAP 4096 // target points resident in LDS (48 KiB as three float arrays)
#define ICP3_UNR 4     // target points per LDS read of the scan; the tile is padded to a multiple of it
#define ICP3_PB 2      // source points per lane and pass over the target, at most (one LDS read serves both)

static_assert(ICP3_TCAP % ICP3_UNR == 0, "the tile is read ICP3_UNR points at a time");
static_assert(ICP3_NSUM == 16, "point-to-point in 3-D: W, sum p, sum q, sum q p^T");
static_assert(ICP3P_NSUM == 28, "point-to-plane in 3-D: W, the upper triangle of sum F F^T, -sum F e");
static_assert(ICP3P4_NSUM == 15, "4-DoF point-to-plane: W, the upper triangle of the 4 x 4 sum F F^T, -sum F e");
static_assert(ICP3P_PIVOT_RTOL == ICP_PIVOT_RTOL, "one singularity rule for the 2-D and the 3-D point-to-plane systems");

#define ICP3_POINT 0 // sfe_icp_params.minimizer of the three instantiations
#define ICP3_PLANE 2
#define ICP3_PLANE4 3 // point-to-plane with force4DOF: 1
#define N3_TILE 2048 // points per LDS tile of the normals kernel (24 KiB), as P3_TILE of sfe_points3.h

template <int MIN>
struct Icp3Sums {
    static constexpr int N = MIN == ICP3_PLANE ? ICP3P_NSUM : MIN == ICP3_PLANE4 ? ICP3P4_NSUM : ICP3_NSUM;
};

// What the job kernel gets by value: the chain's parameters and, in the EXT builds only, the modules sfe_icp_params has no
// field for (MinDist / MedianDist outlier filters, Bound checker).  The EXT = 0 form is sfe_icp_params and nothing else, so
// the kernel of a chain without those modules has the arguments, the code and the registers it had before they existed.
template <int EXT>
struct Icp3Args {
    sfe_icp_params P;
};
template <>
struct Icp3Args<1> {
    sfe_icp_params P;
    sfe_icp_outliers O;
};
static_assert(sizeof(Icp3Args<0>) == sizeof(sfe_icp_params), "the plain kernel takes sfe_icp_params alone");

// c = a * b, 4 x 4 row-major, every entry (((a0 b0 + a1 b1) + a2 b2) + a3 b3) with each product and sum rounded to float
__device__ __forceinline__ void mat4_mul(const float *a, const float *b, float *c)
{
    float r[16];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float s = f_mul(a[i * 4], b[j]);
            s = f_add(s, f_mul(a[i * 4 + 1], b[4 + j]));
            s = f_add(s, f_mul(a[i * 4 + 2], b[8 + j]));
            s = f_add(s, f_mul(a[i * 4 + 3], b[12 + j]));
            r[i * 4 + j] = s;
        }
#pragma unroll
    for (int i = 0; i < 16; ++i)
        c[i] = r[i];
}

// one row of a 4 x 4 transform on a point: ((a x + b y) + c z) + d, every product and sum rounded to float.  Not s3_move of
// sfe_store3.hip: that is numpy's sgemm rule with fused products, this is the ICP chain's rule (the 2-D kernel's, no fma).
__device__ __forceinline__ float affine3(const float *row, float x, float y, float z)
{
    return f_add(f_add(f_add(f_mul(row[0], x), f_mul(row[1], y)), f_mul(row[2], z)), row[3]);
}

struct Icp3Job {
    long long src_start, tgt_start; // first point of the job's clouds in their pools (a store's pool may pass 2^31 points)
    int n_src, n_tgt;
    long long scratch_off; // offset (in points) of this job's slice of the NN scratch
    long long nrm_off;     // offset (in points) of its target's normals (point-to-plane; jobs on one target share them)
};

template <int NS> // the minimiser's sums: 16, 28 or 15
struct Icp3SharedT {
    float tx[ICP3_TCAP], ty[ICP3_TCAP], tz[ICP3_TCAP];
    double red[ICP_WAVES * NS + NS];
    unsigned hist[256];
    unsigned sel_prefix, sel_k;
    int flag_iterate, flag_status;
    float Ti[16];
    float mean[3];
    float hist_T[ICP_MAX_HIST][12]; // rotation block (9, row-major) and translation (3) of T_iter after every step

    // the dynamic LDS of a launch, so every instantiation that is launched passes the check.  (Only its 64 KiB half can
    // fail: red is declared with the size block_sum<NS> needs, and the first half says so where it is relied on.)
    static constexpr size_t bytes()
    {
        static_assert(sizeof(red) >= sizeof(double) * (ICP_WAVES + 1) * NS && sizeof(Icp3SharedT) <= 64 * 1024,
                      "block_sum<NS> needs (waves + 1) x NS doubles; two workgroups per CU");
        return sizeof(Icp3SharedT);
    }
};

// load target points [base, base + n) of the job (packed float triples), centred on the mean, into the LDS tile (+inf pad)
template <class Icp3Shared>
__device__ __forceinline__ void load_tile3(Icp3Shared &S, const float *__restrict__ tgt, int base, int n)
{
    const float mx = S.mean[0], my = S.mean[1], mz = S.mean[2];
    const int npad = (n + ICP3_UNR - 1) / ICP3_UNR * ICP3_UNR;
    for (int i = threadIdx.x; i < npad; i += ICP_THREADS) {
        float x = INFINITY, y = INFINITY, z = INFINITY;
        if (i < n) {
            const float *t = tgt + 3 * (size_t)(base + i);
            x = f_add(t[0], -mx);
            y = f_add(t[1], -my);
            z = f_add(t[2], -mz);
        }
        S.tx[i] = x;
        S.ty[i] = y;
        S.tz[i] = z;
    }
}

// Exact arg-min over the LDS tile (tn points, global indices from tb) for NP query points per lane: index order and a strict
// '<', so the lowest index wins among equal distances; NaN distances and the +inf pad never win.
template <int NP, class Icp3Shared>
__device__ __forceinline__ void nn3_scan_tile(const Icp3Shared &S, int tn, int tb, const float (&px)[ICP3_PB],
                                              const float (&py)[ICP3_PB], const float (&pz)[ICP3_PB], float (&best)[ICP3_PB],
                                              int (&bi)[ICP3_PB])
{
    const int npad = (tn + ICP3_UNR - 1) / ICP3_UNR * ICP3_UNR;
    for (int j = 0; j < npad; j += ICP3_UNR) {
        const float4 x4 = *reinterpret_cast<const float4 *>(&S.tx[j]); // LDS broadcast reads
        const float4 y4 = *reinterpret_cast<const float4 *>(&S.ty[j]);
        const float4 z4 = *reinterpret_cast<const float4 *>(&S.tz[j]);
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const float d0 = p3_dist2(px[k], py[k], pz[k], x4.x, y4.x, z4.x);
            const float d1 = p3_dist2(px[k], py[k], pz[k], x4.y, y4.y, z4.y);
            const float d2 = p3_dist2(px[k], py[k], pz[k], x4.z, y4.z, z4.z);
            const float d3 = p3_dist2(px[k], py[k], pz[k], x4.w, y4.w, z4.w);
            if (d0 < best[k]) {
                best[k] = d0;
                bi[k] = tb + j;
            }
            if (d1 < best[k]) {
                best[k] = d1;
                bi[k] = tb + j + 1;
            }
            if (d2 < best[k]) {
                best[k] = d2;
                bi[k] = tb + j + 2;
            }
            if (d3 < best[k]) {
                best[k] = d3;
                bi[k] = tb + j + 3;
            }
        }
    }
}

// One lane: solve from the reduced sums, T_iter = T_step * T_iter (to LDS), then the Counter and Differential checkers in
// libpointmatcher's order.  Checker state: nhist / counter / iters in the lane's registers, the history in LDS.  Not inlined:
// the fp64 Jacobi sweeps want more registers than the scan loop, and one lane runs them once per iteration.  MIN picks the
// minimiser's solve (point-to-plane: a system that counts as singular ends the job with SFE_ICP_SINGULAR before anything is
// composed or counted; the 4-DoF form likewise, by its 4 x 4 system); everything behind it is the same code for all.
// EXT: the Bound checker in its place of the list (sfe_icp_outliers.bound_order: the rule of icp_solve_and_check,
// sfe_icp_common.h, with icp3_bound_out for the test).
template <int MIN, int EXT>
__device__ __noinline__ void icp3_solve_and_check(const Icp3Args<EXT> &A, const double (&acc)[Icp3Sums<MIN>::N],
                                                     Icp3SharedT<Icp3Sums<MIN>::N> &S, int &nhist, int &counter, int &iters,
                                                     int &status, int &iterate)
{
    const sfe_icp_params &P = A.P;
    status = SFE_ICP_OK;
    iterate = 1;
    if (acc[0] == 0.0) {
        status = SFE_ICP_NO_POINT;
        return;
    }
    double R[9], t[3];
    if constexpr (MIN == ICP3_PLANE) {
        if (icp3p_solve(acc, R, t)) {
            status = SFE_ICP_SINGULAR;
            return;
        }
    } else if constexpr (MIN == ICP3_PLANE4) {
        if (icp3p_solve4(acc, R, t)) {
            status = SFE_ICP_SINGULAR;
            return;
        }
    } else {
        icp3_solve(acc, R, t);
    }
    const float Ts[16] = {(float)R[0], (float)R[1], (float)R[2], (float)t[0], (float)R[3], (float)R[4], (float)R[5], (float)t[1],
                          (float)R[6], (float)R[7], (float)R[8], (float)t[2], 0.0f,        0.0f,        0.0f,        1.0f};
    float Ti[16], Tn[16];
    for (int i = 0; i < 16; ++i)
        Ti[i] = S.Ti[i];
    mat4_mul(Ts, Ti, Tn);
    for (int i = 0; i < 16; ++i)
        S.Ti[i] = Tn[i];
    ++iters;
    ++counter;
    // Bound: not evaluated when a Counter listed before it has just reached its limit; its status ends the job at once
    // unless a Differential checker listed before it runs first (whose NaN status then wins)
    bool out = false;
    if constexpr (EXT) {
        const sfe_icp_outliers &O = A.O;
        out = O.use_bound && !((O.bound_order & 1) && counter >= P.max_iter) && icp3_bound_out(O, Tn);
        if (out && !(O.bound_order & 2)) {
            status = SFE_ICP_BOUND;
            return;
        }
    }
    if (counter >= P.max_iter) {
        iterate = 0; // CounterTransformationChecker: MaxNumIterationsReached
    } else if (P.use_diff_checker) {
        if (nhist == ICP_MAX_HIST) { // keep a sliding window (only the last smooth_len + 1 entries are read)
            for (int i = 1; i < ICP_MAX_HIST; ++i)
                for (int k = 0; k < 12; ++k)
                    S.hist_T[i - 1][k] = S.hist_T[i][k];
            --nhist;
        }
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c)
                S.hist_T[nhist][3 * r + c] = Tn[4 * r + c];
            S.hist_T[nhist][9 + r] = Tn[4 * r + 3];
        }
        ++nhist;
        // rotations.size() > smoothLength; size counts the init entry (= iters + 1)
        if (iters + 1 > P.smooth_len) {
            double rsum = 0, tsum = 0;
            for (int i = nhist - 1; i >= nhist - P.smooth_len; --i) {
                rsum += icp3_rot_dist(S.hist_T[i], S.hist_T[i - 1]);
                const double dx = (double)S.hist_T[i][9] - S.hist_T[i - 1][9];
                const double dy = (double)S.hist_T[i][10] - S.hist_T[i - 1][10];
                const double dz = (double)S.hist_T[i][11] - S.hist_T[i - 1][11];
                tsum += sqrt((dx * dx + dy * dy) + dz * dz);
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
    if constexpr (EXT) {
        if (out && status == SFE_ICP_OK)
            status = SFE_ICP_BOUND;
    }
}

// block_sum<NV> in two steps, for sums that are accumulated in several passes: the wave sums of the values [OFF, OFF + CNT)
// to their places in s_red (any number of calls that together cover [0, NV)), then the rest of block_sum.  Every value
// is reduced in block_sum's order.
template <int NV, int OFF, int CNT>
__device__ __forceinline__ void block_sum_waves(const double (&v)[CNT], double *s_red)
{
    static_assert(OFF >= 0 && CNT >= 1 && OFF + CNT <= NV, "a part of the NV values");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < CNT; ++i) {
        const double s = wave_sum(v[i]);
        if (lane == 0)
            s_red[wave * NV + OFF + i] = s;
    }
}

template <int NV>
__device__ __forceinline__ void block_sum_finish(double (&v)[NV], double *s_red)
{
    __syncthreads();
    if (threadIdx.x < NV) {
        double s = 0;
        for (int w = 0; w < ICP_WAVES; ++w) // fixed order: deterministic
            s += s_red[w * NV + threadIdx.x];
        s_red[ICP_WAVES * NV + threadIdx.x] = s;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i)
        v[i] = s_red[ICP_WAVES * NV + i];
    __syncthreads();
}

// The reference mean of a target of nt packed points (fp64 accumulation, rounded to float) into mean[0 .. 3) (LDS), by a
// workgroup of ICP_THREADS; red: (waves + 1) x 3 doubles of LDS.  One piece of code for the job kernel and for the kernel
// that centres a target before its normals are taken: both see the same three floats.
__device__ __forceinline__ void icp3_target_mean(const float *__restrict__ tgt, int nt, int tid, double *red, float *mean)
{
    double m[3] = {0, 0, 0};
    for (int i = tid; i < nt; i += ICP_THREADS) {
        const float *t = tgt + 3 * (size_t)i;
        m[0] += t[0];
        m[1] += t[1];
        m[2] += t[2];
    }
    block_sum<3>(m, red);
    if (tid == 0) {
        mean[0] = (float)(m[0] / nt);
        mean[1] = (float)(m[1] / nt);
        mean[2] = (float)(m[2] / nt);
    }
    __syncthreads();
}

// EXT = 1: the kernel of a chain that lists a MinDist or MedianDist outlier filter or a Bound checker (sfe_icp_outliers;
// rules at sfe_icp3_compute_jobs_chain_ext in include/sonarfe.h).  The median is a second radix select over the same finite
// d2; MinDist and the median limit join the kernel's one keep test; Bound runs in icp3_solve_and_check.
template <int MIN, int EXT>
__global__ __launch_bounds__(ICP_THREADS) void icp3_job_kernel(Icp3Args<EXT> A, const Icp3Job *__restrict__ jobs,
                                                               const float *__restrict__ src_all,
                                                               const float *__restrict__ tgt_all,
                                                               const float *__restrict__ guess_all,
                                                               const float *__restrict__ nrm_all,
                                                               float *__restrict__ nn_d2_all, int *__restrict__ nn_idx_all,
                                                               float *__restrict__ T_out, int *__restrict__ status_out,
                                                               int *__restrict__ iters_out)
{
    constexpr int NS = Icp3Sums<MIN>::N;
    using Icp3Shared = Icp3SharedT<NS>;
    const sfe_icp_params &P = A.P;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    Icp3Shared &S = *reinterpret_cast<Icp3Shared *>(smem_raw);

    const Icp3Job J = jobs[blockIdx.x];
    const int ns = J.n_src, nt = J.n_tgt;
    const float *__restrict__ src = src_all + 3 * (size_t)J.src_start;
    const float *__restrict__ tgt = tgt_all + 3 * (size_t)J.tgt_start;
    float *__restrict__ nn_d2 = nn_d2_all + J.scratch_off;
    int *__restrict__ nn_idx = nn_idx_all + J.scratch_off;
    const float *guess = guess_all + 16 * (size_t)blockIdx.x;
    const int tid = threadIdx.x;
    const bool resident = nt <= ICP3_TCAP;

    // ---- reference mean (fp64 accumulation, rounded to float) ----
    icp3_target_mean(tgt, nt, tid, S.red, S.mean);
    const float mx = S.mean[0], my = S.mean[1], mz = S.mean[2];
    if (resident) {
        load_tile3(S, tgt, 0, nt);
        __syncthreads();
    }

    // ---- T0 = translate(-mean) * guess ; T_iter = I ----
    float T0[16];
    {
        const float Tc[16] = {1, 0, 0, -mx, 0, 1, 0, -my, 0, 0, 1, -mz, 0, 0, 0, 1};
        float g[16];
#pragma unroll
        for (int i = 0; i < 16; ++i)
            g[i] = guess[i];
        mat4_mul(Tc, g, T0);
    }
    if (tid == 0) {
        for (int i = 0; i < 16; ++i)
            S.Ti[i] = (i % 5 == 0) ? 1.0f : 0.0f;
        for (int k = 0; k < 12; ++k) // DifferentialTransformationChecker::init pushes the identity
            S.hist_T[0][k] = (k == 0 || k == 4 || k == 8) ? 1.0f : 0.0f;
        S.flag_iterate = 1;
        S.flag_status = SFE_ICP_OK;
    }
    __syncthreads();
    int nhist = 1, counter = 0, iters = 0; // thread 0's

    const float r2_match = f_mul(P.matcher_max_dist, P.matcher_max_dist);
    const float r2_filter = f_mul(P.max_dist_filter, P.max_dist_filter);
    float min2 = 0.0f; // EXT: MinDist^2
    if constexpr (EXT)
        min2 = f_mul(A.O.min_dist, A.O.min_dist);

    while (true) {
        float Ti[12];
#pragma unroll
        for (int i = 0; i < 12; ++i)
            Ti[i] = S.Ti[i];
        // the current point of source point i: T_iter * (T0 * src[i]), every row by affine3 (floats, whatever x, y, z are)
        auto cur_point = [&](int i, auto &x, auto &y, auto &z) {
            const float *s = src + 3 * (size_t)i;
            const float sx = s[0], sy = s[1], sz = s[2];
            const float rx = affine3(T0, sx, sy, sz), ry = affine3(T0 + 4, sx, sy, sz), rz = affine3(T0 + 8, sx, sy, sz);
            x = affine3(Ti, rx, ry, rz);
            y = affine3(Ti + 4, rx, ry, rz);
            z = affine3(Ti + 8, rx, ry, rz);
        };

        // ---- match: exact 1-NN of the current points in the centred target ----
        double nfin_d[1] = {0};
        for (int base = 0; base < ns; base += ICP_THREADS * ICP3_PB) {
            const int np = (ns - base > ICP_THREADS) ? ICP3_PB : 1; // uniform: queries per lane in this pass
            float px[ICP3_PB], py[ICP3_PB], pz[ICP3_PB], best[ICP3_PB];
            int bi[ICP3_PB];
#pragma unroll
            for (int k = 0; k < ICP3_PB; ++k) {
                const int i = base + k * ICP_THREADS + tid;
                float x = 0, y = 0, z = 0;
                if (k < np && i < ns)
                    cur_point(i, x, y, z);
                px[k] = x;
                py[k] = y;
                pz[k] = z;
                best[k] = INFINITY;
                bi[k] = -1;
            }
            for (int tb = 0; tb < nt; tb += ICP3_TCAP) {
                const int tn = min(ICP3_TCAP, nt - tb);
                if (!resident) {
                    __syncthreads();
                    load_tile3(S, tgt, tb, tn);
                    __syncthreads();
                }
                if (np == 1)
                    nn3_scan_tile<1>(S, tn, tb, px, py, pz, best, bi);
                else
                    nn3_scan_tile<ICP3_PB>(S, tn, tb, px, py, pz, best, bi);
            }
#pragma unroll
            for (int k = 0; k < ICP3_PB; ++k) {
                const int i = base + k * ICP_THREADS + tid;
                if (k < np && i < ns) {
                    float d = best[k];
                    int id = bi[k];
                    if (id < 0 || !(d <= r2_match)) { // (id < 0: nothing nearer than +inf, NaN included)
                        id = -1;
                        d = INFINITY;
                    } else {
                        nfin_d[0] += 1.0;
                    }
                    nn_d2[i] = d;
                    nn_idx[i] = id;
                }
            }
        }
        block_sum<1>(nfin_d, S.red); // also orders the nn_d2 / nn_idx stores before the re-reads below
        const unsigned nfin = (unsigned)nfin_d[0];

        // ---- TrimmedDistOutlierFilter limit: exact order statistic by radix select ----
        float limit = INFINITY;
        if (P.use_trimmed_filter) {
            if (nfin == 0) { // "no outlier to filter" (uniform: every thread leaves)
                if (tid == 0)
                    S.flag_status = SFE_ICP_NO_OUTLIER;
                break;
            }
            const unsigned k_sel = (P.trim_ratio >= 1.0f) ? nfin - 1 : (unsigned)f_mul((float)nfin, P.trim_ratio);
            limit = icp_select_kth(S, nn_d2, ns, tid, min(k_sel, nfin - 1));
            __syncthreads();
        }
        // ---- MedianDistOutlierFilter limit (EXT): factor x the median, the same select at rank icp_median_rank ----
        float med_limit = INFINITY;
        if constexpr (EXT) {
            if (A.O.use_median) {
                if (nfin == 0) { // "no outlier to filter" (uniform)
                    if (tid == 0)
                        S.flag_status = SFE_ICP_NO_OUTLIER;
                    break;
                }
                // (the barrier above: every wave has read the trimmed limit out of S.sel_prefix, which this select resets)
                med_limit = f_mul(A.O.median_factor, icp_select_kth(S, nn_d2, ns, tid, icp_median_rank(nfin)));
                __syncthreads(); // (... and the median out of it before anything else writes it)
            }
        }
        // the keep test of a stored pair (id, d): a target point in range that MaxDist, Trimmed and (EXT) MinDist / MedianDist keep
        auto keep = [&](int id, float d) {
            bool ok = id >= 0 && id < nt && (!P.use_max_dist_filter || d <= r2_filter) && (!P.use_trimmed_filter || d <= limit);
            if constexpr (EXT)
                ok = ok && icp_ox_keep(A.O, min2, med_limit, d);
            return ok;
        };
        // the centred target point id: out of the LDS tile where the target is resident
        auto target_point = [&](int id, double (&q)[3]) {
            if (resident) {
                q[0] = S.tx[id];
                q[1] = S.ty[id];
                q[2] = S.tz[id];
            } else {
                const float *t = tgt + 3 * (size_t)id;
                q[0] = f_add(t[0], -mx);
                q[1] = f_add(t[1], -my);
                q[2] = f_add(t[2], -mz);
            }
        };
        // the normal of target point id, gathered from HBM (one per kept pair)
        auto target_normal = [&](int id, double (&n)[3]) {
            const float *nv = nrm_all + 3 * (size_t)(J.nrm_off + id);
            n[0] = nv[0];
            n[1] = nv[1];
            n[2] = nv[2];
        };
        // point-to-plane: e = n . (p - q)
        auto plane_err = [&](int id, const double (&n)[3], const double (&p)[3]) {
            double q[3];
            target_point(id, q);
            return (n[0] * (p[0] - q[0]) + n[1] * (p[1] - q[1])) + n[2] * (p[2] - q[2]);
        };

        // ---- error minimiser: accumulate over kept pairs ----
        double acc[NS];
        if constexpr (MIN == ICP3_PLANE) {
            // F = (p x n, n), e = n . (p - q): A += F F^T (upper triangle, row by row), b -= F e, W += 1.  28 fp64
            // accumulators beside the pair's own values do not fit the 128 registers of a 1024-thread workgroup, so the
            // kept pairs are walked twice: W and the rows of A that begin with p x n (16 sums), then the n n^T block and b
            // (12 sums).  Each sum is reduced exactly as block_sum<28> would reduce it.
            auto pass = [&](auto part) {
                constexpr int PART = decltype(part)::value;
                constexpr int OFF = PART ? 16 : 0, CNT = PART ? 12 : 16;
                double a[CNT];
#pragma unroll
                for (int i = 0; i < CNT; ++i)
                    a[i] = 0;
                for (int i = tid; i < ns; i += ICP_THREADS) {
                    const int id = nn_idx[i];
                    if (!keep(id, nn_d2[i]))
                        continue;
                    double p[3], n[3];
                    cur_point(i, p[0], p[1], p[2]);
                    target_normal(id, n);
                    const double F[6] = {p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0],
                                         n[0],                      n[1],                      n[2]};
                    if constexpr (PART == 0) {
                        a[0] += 1.0;
                        int k = 1;
#pragma unroll
                        for (int r = 0; r < 3; ++r)
#pragma unroll
                            for (int c = r; c < 6; ++c)
                                a[k++] += F[r] * F[c];
                    } else {
                        const double e = plane_err(id, n, p);
                        int k = 0;
#pragma unroll
                        for (int r = 3; r < 6; ++r)
#pragma unroll
                            for (int c = r; c < 6; ++c)
                                a[k++] += F[r] * F[c];
#pragma unroll
                        for (int r = 0; r < 6; ++r)
                            a[6 + r] -= F[r] * e;
                    }
                }
                block_sum_waves<NS, OFF, CNT>(a, S.red);
            };
            pass(std::integral_constant<int, 0>());
            pass(std::integral_constant<int, 1>());
            block_sum_finish<NS>(acc, S.red);
        } else if constexpr (MIN == ICP3_PLANE4) {
            // force4DOF: F = ((p x n)_z, n), the third component of the 6-DoF form's p x n and its n; e as there.  W, the
            // upper triangle of the 4 x 4 F F^T (10) and b (4): 15 accumulators, one pass like point-to-point's 16.
#pragma unroll
            for (int i = 0; i < NS; ++i)
                acc[i] = 0;
            for (int i = tid; i < ns; i += ICP_THREADS) {
                const int id = nn_idx[i];
                if (!keep(id, nn_d2[i]))
                    continue;
                double p[3], n[3];
                cur_point(i, p[0], p[1], p[2]);
                target_normal(id, n);
                const double F[4] = {p[0] * n[1] - p[1] * n[0], n[0], n[1], n[2]};
                const double e = plane_err(id, n, p);
                acc[0] += 1.0;
                int k = 1;
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = r; c < 4; ++c)
                        acc[k++] += F[r] * F[c];
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    acc[11 + r] -= F[r] * e;
            }
            block_sum<NS>(acc, S.red);
        } else {
#pragma unroll
            for (int i = 0; i < NS; ++i)
                acc[i] = 0;
            for (int i = tid; i < ns; i += ICP_THREADS) {
                const int id = nn_idx[i];
                if (!keep(id, nn_d2[i]))
                    continue;
                double p[3], q[3];
                cur_point(i, p[0], p[1], p[2]);
                target_point(id, q);
                acc[0] += 1.0;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    acc[1 + a] += p[a];
                    acc[4 + a] += q[a];
#pragma unroll
                    for (int b = 0; b < 3; ++b)
                        acc[7 + 3 * a + b] += q[a] * p[b];
                }
            }
            block_sum<NS>(acc, S.red);
        }

        // ---- solve, compose, check (thread 0) ----
        if (tid == 0) {
            int status, iterate;
            icp3_solve_and_check<MIN, EXT>(A, acc, S, nhist, counter, iters, status, iterate);
            S.flag_status = status;
            S.flag_iterate = (status == SFE_ICP_OK) ? iterate : 0;
        }
        __syncthreads();
        if (!S.flag_iterate)
            break;
    }
    __syncthreads(); // (the break on "no outlier to filter": thread 0's status store before it is read)

    if (tid == 0) {
        const int status = S.flag_status;
        float *To = T_out + 16 * (size_t)blockIdx.x;
        if (status == SFE_ICP_OK) {
            const float Tfwd[16] = {1, 0, 0, mx, 0, 1, 0, my, 0, 0, 1, mz, 0, 0, 0, 1};
            float Ti[16], tmp[16], res[16];
            for (int i = 0; i < 16; ++i)
                Ti[i] = S.Ti[i];
            mat4_mul(Ti, T0, tmp);
            mat4_mul(Tfwd, tmp, res);
            for (int i = 0; i < 16; ++i)
                To[i] = res[i];
        } else {
            for (int i = 0; i < 16; ++i) // pcl.cpp:203,207-210: T stays the guess
                To[i] = guess[i];
        }
        status_out[blockIdx.x] = status;
        iters_out[blockIdx.x] = iters;
    }
}

// ---------------------------------------------------------------------------------------------
// Surface normals of the targets of a point-to-plane call: one table entry per distinct target
// ---------------------------------------------------------------------------------------------
struct Nrm3Target {
    long long start;   // its first point in the pool
    long long nrm_off; // where its normals go (in points)
    int n;             // its points (> 0)
    int pad;
};

// the float mean of every target, exactly as icp3_job_kernel takes it (one workgroup per target)
__global__ __launch_bounds__(ICP_THREADS) void nrm3_mean_kernel(const Nrm3Target *__restrict__ targets,
                                                                const float *__restrict__ pts_all, float *__restrict__ means)
{
    __shared__ double s_red[ICP_WAVES * 3 + 3];
    __shared__ float s_mean[3];
    const Nrm3Target G = targets[blockIdx.x];
    icp3_target_mean(pts_all + 3 * (size_t)G.start, G.n, threadIdx.x, s_red, s_mean);
    if (threadIdx.x < 3)
        means[3 * (size_t)blockIdx.x + threadIdx.x] = s_mean[threadIdx.x];
}

// One lane per point of target blockIdx.y (`first` + blockIdx.y of the table): its k = min(knn, n) nearest points of the
// same target, itself included, in the lexicographic (d2, index) order of match_knn3_kernel (sfe_pcl3.hip) -- a k-slot
// insertion list in registers filled in one pass over the target, which goes through LDS as packed triples, N3_TILE points
// at a time, centred on the target's mean (means == nullptr: as given); a point whose d2 is not below +inf (NaN, infinite
// or overflowing coordinates) is nobody's neighbour, so a list may end short.  Then, in fp64 from the float coordinates in
// list order: the neighbours' mean, C = sum (u - m)(u - m)^T, icp3p_normal (sfe_icp3_plane.h), rounded to float.
__global__ __launch_bounds__(256) void normals3_kernel(const Nrm3Target *__restrict__ targets, int first,
                                                       const float *__restrict__ pts_all, const float *__restrict__ means,
                                                       int knn, float *__restrict__ nrm_all)
{
    __shared__ float s_t[3 * N3_TILE];
    const Nrm3Target G = targets[first + blockIdx.y];
    const int n = G.n;
    if (blockIdx.x * 256 >= n) // (uniform: the whole workgroup leaves before any barrier)
        return;
    const float *__restrict__ pts = pts_all + 3 * (size_t)G.start;
    float mx = 0.0f, my = 0.0f, mz = 0.0f; // (x - 0 = x for every float)
    if (means) {
        mx = means[3 * (size_t)(first + blockIdx.y)];
        my = means[3 * (size_t)(first + blockIdx.y) + 1];
        mz = means[3 * (size_t)(first + blockIdx.y) + 2];
    }
    const int K = min(min(knn, ICP_KMAX), n);
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool act = i < n;
    float qx = 0, qy = 0, qz = 0;
    if (act) {
        qx = f_add(pts[3 * (size_t)i], -mx);
        qy = f_add(pts[3 * (size_t)i + 1], -my);
        qz = f_add(pts[3 * (size_t)i + 2], -mz);
    }
    float bd[ICP_KMAX];
    int bi[ICP_KMAX];
    float kth = INFINITY;
#pragma unroll
    for (int q = 0; q < ICP_KMAX; ++q) {
        bd[q] = INFINITY;
        bi[q] = 0;
    }
    for (int tb = 0; tb < n; tb += N3_TILE) {
        const int tn = min(N3_TILE, n - tb);
        __syncthreads();
        for (int j = threadIdx.x; j < 3 * tn; j += 256) { // consecutive floats: coalesced
            const int a = j % 3;
            s_t[j] = f_add(pts[3 * (size_t)tb + j], -(a == 0 ? mx : a == 1 ? my : mz));
        }
        __syncthreads();
        if (act) {
            for (int j = 0; j < tn; ++j) { // every lane reads the same LDS words: a broadcast
                const float d = p3_dist2(qx, qy, qz, s_t[3 * j], s_t[3 * j + 1], s_t[3 * j + 2]);
                if (d < kth) { // kth = the list's K-th distance (inf until it is full); NaN and inf: never
                    // position = number of kept entries <= d (ascending index: equal distances keep the earlier point)
                    int p = 0;
#pragma unroll
                    for (int q = 0; q < ICP_KMAX; ++q)
                        p += (q < K && bd[q] <= d) ? 1 : 0;
#pragma unroll
                    for (int q = ICP_KMAX - 1; q >= 1; --q) {
                        if (q < K && q > p) {
                            bd[q] = bd[q - 1];
                            bi[q] = bi[q - 1];
                        }
                    }
#pragma unroll
                    for (int q = 0; q < ICP_KMAX; ++q) {
                        if (q == p) {
                            bd[q] = d;
                            bi[q] = tb + j;
                        }
                        if (q == K - 1)
                            kth = bd[q];
                    }
                }
            }
        }
    }
    if (!act)
        return;
    double sx = 0, sy = 0, sz = 0;
    int cnt = 0;
#pragma unroll
    for (int q = 0; q < ICP_KMAX; ++q)
        if (q < K && bd[q] < INFINITY) {
            const float *t = pts + 3 * (size_t)bi[q];
            sx += (double)f_add(t[0], -mx);
            sy += (double)f_add(t[1], -my);
            sz += (double)f_add(t[2], -mz);
            ++cnt;
        }
    double C[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (cnt > 0) {
        sx /= cnt;
        sy /= cnt;
        sz /= cnt;
#pragma unroll
        for (int q = 0; q < ICP_KMAX; ++q)
            if (q < K && bd[q] < INFINITY) {
                const float *t = pts + 3 * (size_t)bi[q];
                const double ux = (double)f_add(t[0], -mx) - sx, uy = (double)f_add(t[1], -my) - sy,
                             uz = (double)f_add(t[2], -mz) - sz;
                C[0] += ux * ux;
                C[1] += ux * uy;
                C[2] += ux * uz;
                C[4] += uy * uy;
                C[5] += uy * uz;
                C[8] += uz * uz;
            }
    }
    double nv[3];
    icp3p_normal(C, nv);
    float *o = nrm_all + 3 * (size_t)(G.nrm_off + i);
    o[0] = (float)nv[0];
    o[1] = (float)nv[1];
    o[2] = (float)nv[2];
}

// The normals of n_targets targets of one pool (table on the device and on the host), enqueue only: the means where the
// ICP centres its targets (d_means != nullptr), then normals3_kernel with the target in blockIdx.y.
static int icp3_normals_dev(sfe_ctx *ctx, const Nrm3Target *d_targets, const Nrm3Target *h_targets, int n_targets,
                            const float *d_pts, float *d_means, int knn, float *d_nrm)
{
    if (d_means)
        hipLaunchKernelGGL(nrm3_mean_kernel, dim3(n_targets), dim3(ICP_THREADS), 0, ctx->stream, d_targets, d_pts, d_means);
    for (int first = 0; first < n_targets; first += 65535) { // (blockIdx.y)
        const int m = std::min(65535, n_targets - first);
        int max_n = 1;
        for (int k = 0; k < m; ++k)
            max_n = std::max(max_n, h_targets[first + k].n);
        hipLaunchKernelGGL(normals3_kernel, dim3((unsigned)((max_n + 255) / 256), (unsigned)m), dim3(256), 0, ctx->stream,
                           d_targets, first, d_pts, (const float *)d_means, knn, d_nrm);
    }
    SFE_LAUNCH_CHECK(ctx);
    return 0;
}

int sfe_icp3_check_params(sfe_ctx *ctx, const sfe_icp_params *p)
{
    SFE_ARG(ctx, p != nullptr);
    if (p->minimizer != ICP3_POINT && p->minimizer != ICP3_PLANE && p->minimizer != ICP3_PLANE4)
        return sfe_set_err(ctx, SFE_ERR_ARG, "3-D ICP runs the point-to-point error minimiser (0) and the 3-D point-to-plane one "
                                             "(2, force2D: 0; 3, force4DOF: 1), not minimizer = %d", p->minimizer);
    SFE_ARG(ctx, p->minimizer == ICP3_POINT || (p->normals_knn >= 2 && p->normals_knn <= ICP_KMAX));
    SFE_ARG(ctx, p->max_iter >= 1);
    SFE_ARG(ctx, !p->use_diff_checker || (p->smooth_len >= 1 && p->smooth_len < ICP_MAX_HIST));
    SFE_ARG(ctx, !p->use_trimmed_filter || (p->trim_ratio >= 0.0f && p->trim_ratio <= 1.0f));
    SFE_ARG(ctx, p->matcher_max_dist > 0.0f);
    return 0;
}

// Enqueue icp3_job_kernel<MIN, EXT> for a staged job table.  One signature for all six, so that sfe_icp3_run_dev picks one
// from a table: the EXT = 0 builds leave `o` alone and pass sfe_icp_params and nothing else.
template <int MIN, int EXT>
static int icp3_launch(sfe_ctx *ctx, const sfe_icp_params &p, const sfe_icp_outliers &o, int n_jobs, const Icp3Job *d_jobs,
                       const float *d_src, const float *d_tgt, const float *d_g, const float *d_nrm, float *d_nn_d2,
                       int *d_nn_idx, float *d_T, int32_t *d_st)
{
    using Shared = Icp3SharedT<Icp3Sums<MIN>::N>;
    Icp3Args<EXT> A{p};
    if constexpr (EXT)
        A.O = o;
    SFE_HIP(ctx, hipFuncSetAttribute((const void *)icp3_job_kernel<MIN, EXT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)Shared::bytes()));
    hipLaunchKernelGGL((icp3_job_kernel<MIN, EXT>), dim3(n_jobs), dim3(ICP_THREADS), Shared::bytes(), ctx->stream, A, d_jobs,
                       d_src, d_tgt, d_g, d_nrm, d_nn_d2, d_nn_idx, d_T, d_st, d_st + n_jobs);
    return 0;
}

// The launch both entry points share (sfe_icp3_compute_jobs on clouds it has just copied up, sfe_icp3_store_compute on a
// store's pool): a validated job table over two device pools, host guesses and host results.  Stages [guesses | job table
// | target table], launches icp3_job_kernel -- for point-to-plane behind the normals of the call's distinct targets (by
// first point and size: the 30 guesses of a compute_batch, or store pairs on one handle, take them once), in stream order
// -- and brings [T | status | iterations] back: one copy each way, one synchronisation.  `o` (nullable; all zero: none)
// names the modules of the EXT build; without any the launch is the plain kernel's.
int sfe_icp3_run_dev(sfe_ctx *ctx, const sfe_icp_params *p, const sfe_icp_outliers *o, const float *d_src,
                     const float *d_tgt, const int64_t *jobs4, const float *guesses16, int n_jobs, float *T_out16,
                     int32_t *status, int32_t *iters)
{
    const bool plane = p->minimizer == ICP3_PLANE || p->minimizer == ICP3_PLANE4; // the minimisers that take normals
    const bool ext = o && (o->use_min_dist || o->use_median || o->use_bound);
    // icp3_launch<MIN, EXT> by [minimiser][EXT].  sfe_icp3_check_params has let 0, 2 and 3 through; the row agrees with
    // `plane` for any value (the point-to-point row is the one that takes no normals).
    static constexpr decltype(&icp3_launch<ICP3_POINT, 0>) launch[3][2] = {
        {icp3_launch<ICP3_POINT, 0>, icp3_launch<ICP3_POINT, 1>},
        {icp3_launch<ICP3_PLANE, 0>, icp3_launch<ICP3_PLANE, 1>},
        {icp3_launch<ICP3_PLANE4, 0>, icp3_launch<ICP3_PLANE4, 1>}};
    const int min_row = p->minimizer == ICP3_PLANE ? 1 : p->minimizer == ICP3_PLANE4 ? 2 : 0;
    std::vector<Icp3Job> jobs((size_t)n_jobs);
    std::vector<Nrm3Target> targets;
    std::map<std::pair<long long, int>, long long> seen; // (first point, size) of a target -> where its normals go
    long long soff = 0, noff = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const int64_t *q = jobs4 + 4 * (size_t)j;
        long long at = 0;
        if (plane) {
            const auto ins = seen.emplace(std::make_pair((long long)q[2], (int)q[3]), noff);
            if (ins.second) {
                targets.push_back({(long long)q[2], noff, (int)q[3], 0});
                noff += q[3];
            }
            at = ins.first->second;
        }
        jobs[j] = {(long long)q[0], (long long)q[2], (int)q[1], (int)q[3], soff, at};
        soff += q[1];
    }
    const int n_targets = (int)targets.size();
    const size_t b_g = sizeof(float) * 16 * (size_t)n_jobs, b_st = sizeof(int32_t) * (size_t)n_jobs, b_out = b_g + 2 * b_st;
    const size_t b_jobs = sizeof(Icp3Job) * (size_t)n_jobs, b_tg = sizeof(Nrm3Target) * (size_t)n_targets;
    float *d_g = (float *)sfe_scratch(ctx, 2, b_g);
    char *d_out = (char *)sfe_scratch(ctx, 3, b_out);
    Icp3Job *d_jobs = (Icp3Job *)sfe_scratch(ctx, 4, b_jobs);
    float *d_nn_d2 = (float *)sfe_scratch(ctx, 5, sizeof(float) * (size_t)soff);
    int *d_nn_idx = (int *)sfe_scratch(ctx, 6, sizeof(int) * (size_t)soff);
    // pinned blocks both ways: [guesses | job table | target table] up, [T | status | iterations] down
    char *h_in = (char *)sfe_pinned_io(ctx, 2, b_g + b_jobs + b_tg);
    char *h_out = (char *)sfe_pinned_io(ctx, 3, b_out);
    if (!d_g || !d_out || !d_jobs || !d_nn_d2 || !d_nn_idx || !h_in || !h_out)
        return SFE_ERR_HIP;
    memcpy(h_in, guesses16, b_g);
    memcpy(h_in + b_g, jobs.data(), b_jobs);
    SFE_HIP(ctx, hipMemcpyAsync(d_g, h_in, b_g, hipMemcpyHostToDevice, ctx->stream));
    SFE_HIP(ctx, hipMemcpyAsync(d_jobs, h_in + b_g, b_jobs, hipMemcpyHostToDevice, ctx->stream));
    int32_t *d_st = (int32_t *)(d_out + b_g);
    float *d_nrm = nullptr;
    if (plane) {
        // normals: 3 floats per point of every distinct target (HBM); [target table | means] in one slot
        d_nrm = (float *)sfe_scratch(ctx, 7, sizeof(float) * 3 * (size_t)noff);
        char *d_tg = (char *)sfe_scratch(ctx, 8, b_tg + sizeof(float) * 3 * (size_t)n_targets);
        if (!d_nrm || !d_tg)
            return SFE_ERR_HIP;
        memcpy(h_in + b_g + b_jobs, targets.data(), b_tg);
        SFE_HIP(ctx, hipMemcpyAsync(d_tg, h_in + b_g + b_jobs, b_tg, hipMemcpyHostToDevice, ctx->stream));
        if (int rc = icp3_normals_dev(ctx, (const Nrm3Target *)d_tg, targets.data(), n_targets, d_tgt, (float *)(d_tg + b_tg),
                                      p->normals_knn, d_nrm))
            return rc;
    }
    if (int rc = launch[min_row][ext](ctx, *p, ext ? *o : sfe_icp_outliers{}, n_jobs, d_jobs, d_src, d_tgt, d_g, d_nrm, d_nn_d2,
                                      d_nn_idx, (float *)d_out, d_st))
        return rc;
    SFE_LAUNCH_CHECK(ctx);
    SFE_HIP(ctx, hipMemcpyAsync(h_out, d_out, b_out, hipMemcpyDeviceToHost, ctx->stream));
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(T_out16, h_out, b_g);
    memcpy(status, h_out + b_g, b_st);
    if (iters)
        memcpy(iters, h_out + b_g + b_st, b_st);
    return 0;
}

extern "C" {

int sfe_icp3_compute_jobs(sfe_ctx *ctx, const sfe_icp_params *p, const float *src, int n_src_pts, const float *tgt,
                          int n_tgt_pts, const int32_t *jobs4, const float *guesses16, int n_jobs, float *T_out16,
                          int32_t *status, int32_t *iters)
{
    return sfe_icp3_compute_jobs_chain_ext(ctx, p, nullptr, nullptr, 0, nullptr, 0, src, n_src_pts, tgt, n_tgt_pts, jobs4,
                                           guesses16, n_jobs, T_out16, status, iters);
}

int sfe_icp3_compute_jobs_chain_ext(sfe_ctx *ctx, const sfe_icp_params *p, const sfe_icp_outliers *o, const sfe_icp_dpf *rd,
                                    int n_rd, const sfe_icp_dpf *rf, int n_rf, const float *src, int n_src_pts,
                                    const float *tgt, int n_tgt_pts, const int32_t *jobs4, const float *guesses16, int n_jobs,
                                    float *T_out16, int32_t *status, int32_t *iters)
{
    if (int rc = sfe_use(ctx))
        return rc;
    if (int rc = sfe_icp3_check_params(ctx, p))
        return rc;
    if (int rc = sfe_icp3_check_chain(ctx, o, rd, n_rd, rf, n_rf))
        return rc;
    SFE_ARG(ctx, n_jobs >= 0 && n_src_pts >= 0 && n_tgt_pts >= 0 &&
                     (n_jobs == 0 || (src && tgt && jobs4 && guesses16 && T_out16 && status)));
    if (n_jobs == 0)
        return 0;
    std::vector<int64_t> jobs((size_t)n_jobs * 4);
    for (int j = 0; j < n_jobs; ++j) {
        const int32_t *q = jobs4 + 4 * (size_t)j;
        if (q[0] < 0 || q[1] <= 0 || q[2] < 0 || q[3] <= 0 || (long long)q[0] + q[1] > n_src_pts ||
            (long long)q[2] + q[3] > n_tgt_pts)
            return sfe_set_err(ctx, SFE_ERR_ARG, "3-D ICP job %d (%d+%d, %d+%d) is empty or lies outside the clouds (%d, %d points)",
                               j, q[0], q[1], q[2], q[3], n_src_pts, n_tgt_pts);
        for (int k = 0; k < 4; ++k)
            jobs[4 * (size_t)j + k] = q[k];
    }
    const size_t b_src = sizeof(float) * 3 * (size_t)n_src_pts, b_tgt = sizeof(float) * 3 * (size_t)n_tgt_pts;
    float *d_src = (float *)sfe_scratch(ctx, 0, b_src);
    float *d_tgt = (float *)sfe_scratch(ctx, 1, b_tgt);
    if (!d_src || !d_tgt)
        return SFE_ERR_HIP;
    SFE_HIP(ctx, hipMemcpyAsync(d_src, src, b_src, hipMemcpyHostToDevice, ctx->stream));
    SFE_HIP(ctx, hipMemcpyAsync(d_tgt, tgt, b_tgt, hipMemcpyHostToDevice, ctx->stream));
    return sfe_icp3_chain_run_dev(ctx, p, o, rd, n_rd, rf, n_rf, d_src, d_tgt, jobs.data(), guesses16, n_jobs, T_out16, status,
                                  iters);
}

int sfe_normals3(sfe_ctx *ctx, const float *pts, int n, int knn, float *normals_out)
{
    if (int rc = sfe_use(ctx))
        return rc;
    SFE_ARG(ctx, n >= 0 && n <= (1 << 28) && knn >= 2 && knn <= ICP_KMAX && (n == 0 || (pts && normals_out)));
    if (n == 0)
        return 0;
    const size_t b_pts = sizeof(float) * 3 * (size_t)n;
    float *d_pts = (float *)sfe_scratch(ctx, 0, b_pts);
    float *d_nrm = (float *)sfe_scratch(ctx, 7, b_pts);
    Nrm3Target *d_tg = (Nrm3Target *)sfe_scratch(ctx, 8, sizeof(Nrm3Target));
    Nrm3Target *h_tg = (Nrm3Target *)sfe_pinned_io(ctx, 2, sizeof(Nrm3Target));
    if (!d_pts || !d_nrm || !d_tg || !h_tg)
        return SFE_ERR_HIP;
    *h_tg = {0, 0, n, 0};
    SFE_HIP(ctx, hipMemcpyAsync(d_pts, pts, b_pts, hipMemcpyHostToDevice, ctx->stream));
    SFE_HIP(ctx, hipMemcpyAsync(d_tg, h_tg, sizeof(Nrm3Target), hipMemcpyHostToDevice, ctx->stream));
    if (int rc = icp3_normals_dev(ctx, d_tg, h_tg, 1, d_pts, nullptr, knn, d_nrm)) // the cloud as given: no centring
        return rc;
    SFE_HIP(ctx, hipMemcpyAsync(normals_out, d_nrm, b_pts, hipMemcpyDeviceToHost, ctx->stream));
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

} // extern "C"
