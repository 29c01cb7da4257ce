// Data-point filters of a libpointmatcher ICP chain (readingDataPointsFilters / referenceDataPointsFilters of
// icp.yaml) on gfx950, as a pass in front of the ICP launch (sfe_icp.hip / sfe_icp_sweep.hip, unchanged).
//
// What libpointmatcher's ICP::compute / computeWithTransformedReference does with them (restated from its published
// source, UNPINNED like the rest of pcl.cpp's third-party behaviour): the reading filters run once on the reading in
// its own frame, before the guess is applied; the reference filters run once on the reference in its own frame, and
// the reference mean used for centring is taken from the filtered reference.  So ICP with a filter chain is ICP on the
// filtered clouds, which is how it runs here: every distinct cloud of a call is filtered once, and the ICP job table is
// built on the filtered pools.
//
// Stages (include/sonarfe.h, SFE_DPF_*):
//   * predicates (MaxDist, MinDist, BoundingBox): a run of consecutive predicate stages is ONE pass, one workgroup per
//     cloud, the stages evaluated together per point.  The order of the kept points comes from a ballot / popcount
//     prefix inside each wave and a scan of the wave totals across the workgroup, carried from chunk to chunk: no
//     atomic decides a position.  Every product / sum is rounded to float (f_mul / f_add) and the norm goes through the
//     correctly rounded sqrtf, so a point one ulp either side of a threshold falls the way the float restatement says.
//   * OctreeGridDataPointsFilter {samplingMethod: 3}: the medoid octree of pcl.downsample, run by the resident batch
//     filter (sfe_cloudfilter.hip) on the clouds staged at a common capacity: LDS sorts for clouds of <= 16384 points,
//     the HBM-scratch sort beyond.  Output = sfe_downsample's, point for point; a tree deeper than 24 levels gives -1.
//
// Scratch slots 64-71 (the ICP launch uses 0-24 and 30-62, the cloud filter 25-29, 31, 40, 52 and 63).
#include "sfe_cloudfilter.h"
#include "sfe_icp_common.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <utility>

#define DPF_THREADS 256 // one workgroup per cloud for the predicate pass
#define DPF_UNROLL 4    // points per thread in flight per chunk (DPF_THREADS * DPF_UNROLL per chunk)
#define DPF_SLOT_SRC 64 // filtered reading pool (ICP chain)
#define DPF_SLOT_TGT 65 // filtered reference pool (ICP chain)
#define DPF_SLOT_A 66   // ping-pong between stage groups
#define DPF_SLOT_B 67
#define DPF_SLOT_TAB 68 // per-cloud tables: input offsets, output offsets, counts (x 2)
#define DPF_SLOT_OCT 69 // octree stage output, [cloud][cap]
#define DPF_SLOT_PACK 70 // sfe_icp_filter_clouds_dev: before packing
#define DPF_SLOT_OCNT 71 // octree stage counts

struct DpfPreds {
    int n;
    sfe_icp_dpf s[SFE_DPF_MAX_STAGES];
};

__device__ __forceinline__ bool dpf_keep(const sfe_icp_dpf &s, float x, float y)
{
    if (s.kind == SFE_DPF_BOUNDING_BOX) {
        const bool inside = s.f[0] < x && x < s.f[1] && s.f[2] < y && y < s.f[3];
        return inside != (s.remove_inside != 0);
    }
    const bool max = s.kind == SFE_DPF_MAX_DIST;
    if (s.dim < 0) {
        const float norm = sqrtf(f_add(f_mul(x, x), f_mul(y, y)));
        return max ? norm < fabsf(s.f[0]) : norm > fabsf(s.f[0]);
    }
    const float v = s.dim == 0 ? x : y;
    return max ? v < s.f[0] : fabsf(v) > fabsf(s.f[0]);
}

// one workgroup per cloud: cloud c = src[in_off[c] .. + in_cnt[c]) -> dst[out_off[c] ..), out_cnt[c] kept points
// (in_cnt[c] < 0: a refused cloud stays refused)
__global__ __launch_bounds__(DPF_THREADS) void dpf_predicate_kernel(DpfPreds L, const float2 *__restrict__ src,
                                                                    const long long *__restrict__ in_off,
                                                                    const int *__restrict__ in_cnt,
                                                                    float2 *__restrict__ dst,
                                                                    const long long *__restrict__ out_off,
                                                                    int *__restrict__ out_cnt)
{
    __shared__ int s_wave[DPF_UNROLL][DPF_THREADS / 64];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = in_cnt[c];
    if (n < 0) {
        if (tid == 0)
            out_cnt[c] = -1;
        return;
    }
    const float2 *p = src + in_off[c];
    float2 *o = dst + out_off[c];
    const unsigned long long below = (1ull << lane) - 1ull;
    int carry = 0;
    for (int base = 0; base < n; base += DPF_THREADS * DPF_UNROLL) {
        float2 q[DPF_UNROLL];
        bool keep[DPF_UNROLL];
#pragma unroll
        for (int u = 0; u < DPF_UNROLL; ++u) {
            const int i = base + u * DPF_THREADS + tid;
            keep[u] = i < n;
            q[u] = keep[u] ? p[i] : make_float2(0.0f, 0.0f);
        }
        int at[DPF_UNROLL];
#pragma unroll
        for (int u = 0; u < DPF_UNROLL; ++u) {
            for (int s = 0; s < L.n; ++s)
                keep[u] = keep[u] && dpf_keep(L.s[s], q[u].x, q[u].y);
            const unsigned long long m = __ballot(keep[u]);
            at[u] = __popcll(m & below);
            if (lane == 0)
                s_wave[u][wave] = __popcll(m);
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < DPF_UNROLL; ++u) {
            int off = carry;
            for (int v = 0; v < u; ++v)
                for (int w = 0; w < DPF_THREADS / 64; ++w)
                    off += s_wave[v][w];
            for (int w = 0; w < wave; ++w)
                off += s_wave[u][w];
            if (keep[u])
                o[off + at[u]] = q[u];
        }
        for (int u = 0; u < DPF_UNROLL; ++u)
            for (int w = 0; w < DPF_THREADS / 64; ++w)
                carry += s_wave[u][w];
        __syncthreads();
    }
    if (tid == 0)
        out_cnt[c] = carry;
}

// one workgroup per cloud: stage the cloud at [c][cap] for the resident octree filter, with its root and depth
// (cf_cast_bbox_kernel's work on float32 input at variable offsets)
__global__ __launch_bounds__(1024) void dpf_octree_stage_kernel(const float2 *__restrict__ src,
                                                                const long long *__restrict__ in_off,
                                                                const int *__restrict__ in_cnt, long long cap,
                                                                float max_size, float2 *__restrict__ p32,
                                                                CfHeader *__restrict__ hdrs)
{
    __shared__ float s_mn[2][16], s_mx[2][16];
    const int c = blockIdx.x;
    const int n = max(in_cnt[c], 0);
    const float2 *p = src + in_off[c];
    float2 *d = p32 + (size_t)c * cap;
    float mnx = INFINITY, mny = INFINITY, mxx = -INFINITY, mxy = -INFINITY;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const float2 q = p[i];
        d[i] = q;
        mnx = fminf(mnx, q.x);
        mxx = fmaxf(mxx, q.x);
        mny = fminf(mny, q.y);
        mxy = fmaxf(mxy, q.y);
    }
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) {
        mnx = fminf(mnx, __shfl_down(mnx, k));
        mxx = fmaxf(mxx, __shfl_down(mxx, k));
        mny = fminf(mny, __shfl_down(mny, k));
        mxy = fmaxf(mxy, __shfl_down(mxy, k));
    }
    if ((threadIdx.x & 63) == 0) {
        s_mn[0][threadIdx.x >> 6] = mnx;
        s_mn[1][threadIdx.x >> 6] = mny;
        s_mx[0][threadIdx.x >> 6] = mxx;
        s_mx[1][threadIdx.x >> 6] = mxy;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) {
            mnx = fminf(mnx, s_mn[0][w]);
            mny = fminf(mny, s_mn[1][w]);
            mxx = fmaxf(mxx, s_mx[0][w]);
            mxy = fmaxf(mxy, s_mx[1][w]);
        }
        hdrs[c] = cf_make_header(mnx, mny, mxx, mxy, max_size, n);
    }
}

// one workgroup per cloud: [c][cap] medoids -> dst[out_off[c] ..); a cloud refused before the stage stays refused
__global__ __launch_bounds__(256) void dpf_octree_unstage_kernel(const float2 *__restrict__ ds, long long cap,
                                                                 const int *__restrict__ ds_cnt,
                                                                 const int *__restrict__ in_cnt,
                                                                 float2 *__restrict__ dst,
                                                                 const long long *__restrict__ out_off,
                                                                 int *__restrict__ out_cnt)
{
    const int c = blockIdx.x;
    const int m = in_cnt[c] < 0 ? -1 : ds_cnt[c];
    const float2 *s = ds + (size_t)c * cap;
    float2 *o = dst + out_off[c];
    for (int i = threadIdx.x; i < m; i += 256)
        o[i] = s[i];
    if (threadIdx.x == 0)
        out_cnt[c] = m;
}

// one workgroup per cloud: src[in_off[c] .. + max(cnt[c], 0)) -> dst[out_off[c] ..)
__global__ __launch_bounds__(256) void dpf_pack_kernel(const float2 *__restrict__ src,
                                                       const long long *__restrict__ in_off,
                                                       const int *__restrict__ cnt, float2 *__restrict__ dst,
                                                       const long long *__restrict__ out_off)
{
    const int c = blockIdx.x;
    const int m = cnt[c];
    const float2 *s = src + in_off[c];
    float2 *o = dst + out_off[c];
    for (int i = threadIdx.x; i < m; i += 256)
        o[i] = s[i];
}

int sfe_icp_dpf_check(sfe_ctx *ctx, const sfe_icp_dpf *st, int n)
{
    SFE_ARG(ctx, n >= 0 && n <= SFE_DPF_MAX_STAGES && (n == 0 || st));
    for (int i = 0; i < n; ++i) {
        const sfe_icp_dpf &s = st[i];
        if (s.kind == SFE_DPF_MAX_DIST || s.kind == SFE_DPF_MIN_DIST) {
            if (s.dim < -1 || s.dim > 1)
                return sfe_set_err(ctx, SFE_ERR_ARG, "data-point filter stage %d: dim %d is not -1, 0 or 1 (2-D clouds)",
                                   i, s.dim);
        } else if (s.kind == SFE_DPF_OCTREE_GRID) {
            if (!(s.f[0] > 0.0f) || !std::isfinite(s.f[0]))
                return sfe_set_err(ctx, SFE_ERR_ARG, "data-point filter stage %d: maxSizeByNode %g is not > 0", i,
                                   (double)s.f[0]);
        } else if (s.kind != SFE_DPF_BOUNDING_BOX) {
            return sfe_set_err(ctx, SFE_ERR_ARG, "data-point filter stage %d: unknown kind %d", i, s.kind);
        }
    }
    return 0;
}

// The stages over n_clouds clouds: cloud c = d_in[in_off[c] .. + n[c]) -> d_out[out_off[c] ..) (room for n[c] points
// each), kept counts to h_counts (host, one synchronisation; -1: octree deeper than 24 levels).  Stage groups alternate
// between two scratch buffers laid out like d_out; the last group writes d_out.
static int dpf_run(sfe_ctx *ctx, const sfe_icp_dpf *st, int n_st, const float2 *d_in, const long long *in_off,
                   const int32_t *n, int n_clouds, float2 *d_out, const long long *out_off, int32_t *h_counts)
{
    long long total = 0;
    int cap = 1;
    for (int c = 0; c < n_clouds; ++c) {
        total = std::max(total, out_off[c] + n[c]);
        cap = std::max(cap, (int)n[c]);
    }
    bool has_octree = false;
    for (int i = 0; i < n_st; ++i)
        has_octree |= st[i].kind == SFE_DPF_OCTREE_GRID;
    if (has_octree && cap > CF_MAX_CAP)
        return sfe_set_err(ctx, SFE_ERR_ARG, "OctreeGridDataPointsFilter on a cloud of %d points (at most %d)", cap,
                           CF_MAX_CAP);
    // [in_off | out_off] as long long, then [count ping | count pong] as int
    const size_t nc = (size_t)n_clouds, b_tab = 16 * nc + 8 * nc;
    char *d_tab = (char *)sfe_scratch(ctx, DPF_SLOT_TAB, b_tab);
    float2 *d_a = (float2 *)sfe_scratch(ctx, DPF_SLOT_A, sizeof(float2) * (size_t)std::max(total, 1LL));
    float2 *d_b = (float2 *)sfe_scratch(ctx, DPF_SLOT_B, sizeof(float2) * (size_t)std::max(total, 1LL));
    if (!d_tab || !d_a || !d_b)
        return SFE_ERR_HIP;
    long long *d_in_off = (long long *)d_tab, *d_out_off = d_in_off + nc;
    int *d_cnt[2] = {(int *)(d_out_off + nc), (int *)(d_out_off + nc) + nc};
    {
        char *h = (char *)sfe_pinned_begin(ctx, b_tab);
        if (!h)
            return SFE_ERR_HIP;
        memcpy(h, in_off, 8 * nc);
        memcpy(h + 8 * nc, out_off, 8 * nc);
        memcpy(h + 16 * nc, n, 4 * nc);
        SFE_HIP(ctx, hipMemcpyAsync(d_tab, h, 20 * nc, hipMemcpyHostToDevice, ctx->stream));
        if (int rc = sfe_pinned_end(ctx, ctx->stream))
            return rc;
    }
    // stage groups: a run of predicates, or one octree stage
    std::vector<std::pair<int, int>> groups;
    for (int i = 0; i < n_st;) {
        int j = i + 1;
        if (st[i].kind != SFE_DPF_OCTREE_GRID)
            while (j < n_st && st[j].kind != SFE_DPF_OCTREE_GRID)
                ++j;
        groups.emplace_back(i, j);
        i = j;
    }
    const float2 *cur = d_in;
    const long long *cur_off = d_in_off;
    int ci = 0; // d_cnt[ci] holds the current counts
    for (size_t g = 0; g < groups.size(); ++g) {
        float2 *nxt = g + 1 == groups.size() ? d_out : (g & 1 ? d_b : d_a);
        const int i0 = groups[g].first, i1 = groups[g].second;
        if (st[i0].kind != SFE_DPF_OCTREE_GRID) {
            DpfPreds L{};
            L.n = i1 - i0;
            for (int i = i0; i < i1; ++i)
                L.s[i - i0] = st[i];
            hipLaunchKernelGGL(dpf_predicate_kernel, dim3(n_clouds), dim3(DPF_THREADS), 0, ctx->stream, L, cur, cur_off,
                               d_cnt[ci], nxt, d_out_off, d_cnt[ci ^ 1]);
        } else {
            ctx->staged_frames = -1; // (the cloud filter's staging slots are rewritten)
            float2 *d_p32 = (float2 *)sfe_scratch(ctx, CF_SLOT_P32, sizeof(float2) * (size_t)cap * nc);
            CfHeader *d_hdr = (CfHeader *)sfe_scratch(ctx, CF_SLOT_HDR, sizeof(CfHeader) * nc);
            float2 *d_ds = (float2 *)sfe_scratch(ctx, DPF_SLOT_OCT, sizeof(float2) * (size_t)cap * nc);
            int *d_ds_cnt = (int *)sfe_scratch(ctx, DPF_SLOT_OCNT, sizeof(int) * nc);
            if (!d_p32 || !d_hdr || !d_ds || !d_ds_cnt)
                return SFE_ERR_HIP;
            const float res = st[i0].f[0];
            hipLaunchKernelGGL(dpf_octree_stage_kernel, dim3(n_clouds), dim3(1024), 0, ctx->stream, cur, cur_off,
                               d_cnt[ci], (long long)cap, sfe_cf_max_size(res), d_p32, d_hdr);
            if (int rc = sfe_cf_run_staged(ctx, n_clouds, cap, res, 0.0, 0, (float *)d_ds, d_ds_cnt))
                return rc;
            hipLaunchKernelGGL(dpf_octree_unstage_kernel, dim3(n_clouds), dim3(256), 0, ctx->stream, d_ds, (long long)cap,
                               d_ds_cnt, d_cnt[ci], nxt, d_out_off, d_cnt[ci ^ 1]);
        }
        SFE_LAUNCH_CHECK(ctx);
        cur = nxt;
        cur_off = d_out_off;
        ci ^= 1;
    }
    if (groups.empty()) // no stage: a copy
        hipLaunchKernelGGL(dpf_pack_kernel, dim3(n_clouds), dim3(256), 0, ctx->stream, d_in, d_in_off, d_cnt[0], d_out,
                           d_out_off);
    SFE_LAUNCH_CHECK(ctx);
    SFE_HIP(ctx, hipMemcpyAsync(h_counts, d_cnt[ci], 4 * nc, hipMemcpyDeviceToHost, ctx->stream));
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// distinct (start, n) slices of a job table's source (col 0) or target (col 2) side, in first-use order
struct DpfSlices {
    std::vector<long long> start, base; // input offset, offset in the filtered pool
    std::vector<int32_t> n, kept;
    std::vector<int> of_job;
};
static void dpf_slices(const int32_t *jobs4, int n_jobs, int col, DpfSlices &s)
{
    std::map<std::pair<int, int>, int> seen;
    s.of_job.resize((size_t)n_jobs);
    long long off = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const int32_t *q = jobs4 + 4 * (size_t)j + col;
        const auto key = std::make_pair((int)q[0], (int)q[1]);
        auto it = seen.find(key);
        if (it == seen.end()) {
            it = seen.emplace(key, (int)s.n.size()).first;
            s.start.push_back(q[0]);
            s.n.push_back(q[1]);
            s.base.push_back(off);
            off += q[1];
        }
        s.of_job[j] = it->second;
    }
    s.kept.assign(s.n.size(), 0);
}

// The chain on a job table over device pools (d_src / d_tgt hold the clouds, jobs4 validated), guesses on the host;
// results to the host.
int sfe_icp_dpf_run_host(sfe_ctx *ctx, const sfe_icp_params *p, const IcpCall &call, const sfe_icp_dpf *rd, int n_rd,
                         const sfe_icp_dpf *rf, int n_rf, const float *d_src, const float *d_tgt, const int32_t *jobs4,
                         const float *guesses9, int n_jobs, float *T_out9, int32_t *status, int32_t *iters)
{
    // (the filters run in front of the launch that checks the parameters: a minimiser the 2-D kernels do not have -- 2, the
    // 3-D point-to-plane one -- is refused before they do)
    SFE_ARG(ctx, p != nullptr && (p->minimizer == 0 || p->minimizer == 1));
    DpfSlices S, R;
    dpf_slices(jobs4, n_jobs, 0, S);
    dpf_slices(jobs4, n_jobs, 2, R);
    const float *fsrc = d_src, *ftgt = d_tgt;
    // (the filtered pools live in slots the ICP launch does not touch)
    for (int side = 0; side < 2; ++side) {
        DpfSlices &D = side ? R : S;
        const sfe_icp_dpf *st = side ? rf : rd;
        const int n_st = side ? n_rf : n_rd;
        if (n_st == 0) {
            D.base = D.start;
            D.kept = D.n;
            continue;
        }
        const long long total = D.base.back() + D.n.back();
        float2 *d_f = (float2 *)sfe_scratch(ctx, side ? DPF_SLOT_TGT : DPF_SLOT_SRC, sizeof(float2) * (size_t)total);
        if (!d_f)
            return SFE_ERR_HIP;
        if (int rc = dpf_run(ctx, st, n_st, (const float2 *)(side ? d_tgt : d_src), D.start.data(), D.n.data(),
                             (int)D.n.size(), d_f, D.base.data(), D.kept.data()))
            return rc;
        (side ? ftgt : fsrc) = (const float *)d_f;
    }
    // the ICP job table on the filtered pools; jobs with a refused or empty cloud never reach a kernel
    std::vector<int32_t> jobs, idx;
    std::vector<float> g;
    for (int j = 0; j < n_jobs; ++j) {
        const int a = S.of_job[j], b = R.of_job[j];
        const int ns = S.kept[a], nt = R.kept[b];
        memcpy(T_out9 + 9 * (size_t)j, guesses9 + 9 * (size_t)j, sizeof(float) * 9);
        if (iters)
            iters[j] = 0;
        if (ns < 0 || nt < 0) {
            status[j] = SFE_ICP_DPF_DEPTH;
        } else if (ns == 0 || nt == 0) {
            status[j] = SFE_ICP_DPF_EMPTY;
        } else {
            idx.push_back(j);
            const int32_t q[4] = {(int32_t)S.base[a], ns, (int32_t)R.base[b], nt};
            jobs.insert(jobs.end(), q, q + 4);
            g.insert(g.end(), guesses9 + 9 * (size_t)j, guesses9 + 9 * (size_t)j + 9);
        }
    }
    const int m = (int)idx.size();
    std::vector<int8_t> routes((size_t)n_jobs, (int8_t)-1);
    if (m > 0) {
        std::vector<float> T((size_t)m * 9);
        std::vector<int32_t> st((size_t)m * 2);
        if (int rc = sfe_icp_run_host(ctx, p, call, fsrc, ftgt, jobs.data(), g.data(), nullptr, m, T.data(), st.data(),
                                      st.data() + m))
            return rc;
        for (int k = 0; k < m; ++k) {
            const int j = idx[k];
            memcpy(T_out9 + 9 * (size_t)j, T.data() + 9 * (size_t)k, sizeof(float) * 9);
            status[j] = st[k];
            if (iters)
                iters[j] = st[m + k];
            routes[j] = ctx->icp_routes[(size_t)k];
        }
    }
    ctx->icp_routes = routes;
    return 0;
}

extern "C" {

int sfe_icp_filter_clouds_dev(sfe_ctx *ctx, const sfe_icp_dpf *stages, int n_stages, const float *d_pts,
                              const int32_t *off, int n_clouds, float *d_out, int32_t *counts_out)
{
    if (int rc = sfe_use(ctx))
        return rc;
    SFE_ARG(ctx, n_clouds >= 0 && (n_clouds == 0 || (off && d_pts && d_out && counts_out)));
    if (int rc = sfe_icp_dpf_check(ctx, stages, n_stages))
        return rc;
    if (n_clouds == 0)
        return 0;
    std::vector<long long> in_off((size_t)n_clouds), out_off((size_t)n_clouds + 1);
    std::vector<int32_t> n((size_t)n_clouds);
    for (int c = 0; c < n_clouds; ++c) {
        if (off[c] < 0 || off[c + 1] < off[c])
            return sfe_set_err(ctx, SFE_ERR_ARG, "sfe_icp_filter_clouds_dev: off[%d..%d] = %d, %d", c, c + 1, off[c],
                               off[c + 1]);
        in_off[c] = off[c];
        n[c] = off[c + 1] - off[c];
    }
    float2 *d_tmp = (float2 *)sfe_scratch(ctx, DPF_SLOT_PACK, sizeof(float2) * (size_t)std::max(off[n_clouds], 1));
    if (!d_tmp)
        return SFE_ERR_HIP;
    if (int rc = dpf_run(ctx, stages, n_stages, (const float2 *)d_pts, in_off.data(), n.data(), n_clouds, d_tmp,
                         in_off.data(), counts_out))
        return rc;
    // back to back: cloud c after the survivors of the clouds in front of it
    out_off[0] = 0;
    for (int c = 0; c < n_clouds; ++c)
        out_off[c + 1] = out_off[c] + std::max(counts_out[c], 0);
    const size_t nc = (size_t)n_clouds;
    char *d_tab = (char *)sfe_scratch(ctx, DPF_SLOT_TAB, 20 * nc);
    if (!d_tab)
        return SFE_ERR_HIP;
    {
        char *h = (char *)sfe_pinned_begin(ctx, 20 * nc);
        if (!h)
            return SFE_ERR_HIP;
        memcpy(h, in_off.data(), 8 * nc);
        memcpy(h + 8 * nc, out_off.data(), 8 * nc);
        for (size_t c = 0; c < nc; ++c)
            ((int32_t *)(h + 16 * nc))[c] = std::max(counts_out[c], 0);
        SFE_HIP(ctx, hipMemcpyAsync(d_tab, h, 20 * nc, hipMemcpyHostToDevice, ctx->stream));
        if (int rc = sfe_pinned_end(ctx, ctx->stream))
            return rc;
    }
    hipLaunchKernelGGL(dpf_pack_kernel, dim3(n_clouds), dim3(256), 0, ctx->stream, d_tmp, (const long long *)d_tab,
                       (const int *)(d_tab + 16 * nc), (float2 *)d_out, (const long long *)(d_tab + 8 * nc));
    SFE_LAUNCH_CHECK(ctx);
    return 0;
}

} // extern "C"
