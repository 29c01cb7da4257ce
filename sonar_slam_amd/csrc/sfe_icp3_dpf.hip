// Data-point filters of a libpointmatcher ICP chain on N x 3 clouds (readingDataPointsFilters / referenceDataPointsFilters
// of a chain written for 3-D, icp_config.IcpChain with dims = 3) on gfx950, as a pass in front of the 3-D ICP launch
// (sfe_icp3.hip): sfe_icp_dpf.hip with one more coordinate.  ICP with a filter chain is ICP on the filtered clouds: every
// distinct cloud of a call is filtered once, in its own frame, and the job table is rebuilt on the filtered pools.
//
// Clouds are packed float triples.  A call's clouds keep ONE layout through all stages: cloud c owns the points
// [base[c], base[c] + n[c]) of two ping-pong buffers (base = the running sum of the input sizes), its current size lives in
// a device-side job table (S3Job: cat = base[c], tot = the size) that every stage reads and updates, so no stage needs the
// host to know a size and the whole pass synchronises once, at the end, for the counts.
//   * predicates (MaxDist, MinDist, BoundingBox; icp3_dpf_keep of sfe_icp3_chain.h): a run of consecutive predicate stages
//     is ONE pass, one workgroup per cloud, the stages evaluated together per point.  The order of the kept points comes
//     from a ballot / popcount prefix inside each wave and a scan of the wave totals across the workgroup, carried from
//     chunk to chunk: no atomic decides a position.
//   * OctreeGridDataPointsFilter {samplingMethod: 3}: the multi-job downsample of sfe_octree3.hip (bounding box -> keys
//     -> ranks -> segments -> medoids, one launch per step for all clouds), the kernels sfe_downsample3 runs with one job;
//     the tree is cut at 21 levels, so no cloud is ever refused.
//   * the end: the sizes' exclusive sum and the placement back to back, the same file's offsets / place kernels.
//
// Scratch slots 64-70, shared with the 2-D pass of sfe_icp_dpf.hip (a call is one or the other, both end synchronised).
#include "sfe_icp3_chain.h"
#include "sfe_icp_common.h"
#include "sfe_octree3.h"

#include <algorithm>
#include <cstring>
#include <map>
#include <utility>

#define DPF3_THREADS 256 // one workgroup per cloud for the predicate pass
#define DPF3_UNROLL 4    // points per thread in flight per chunk
#define DPF3_SLOT_SRC 64 // filtered reading pool (ICP chain)
#define DPF3_SLOT_TGT 65 // filtered reference pool (ICP chain)
#define DPF3_SLOT_A 66   // ping-pong between stage groups
#define DPF3_SLOT_B 67
#define DPF3_SLOT_TAB 68 // job table, input offsets, bases | output offsets, tree headers, counts
#define DPF3_SLOT_KEYS 69 // octree stage: keys and sorted keys
#define DPF3_SLOT_IDX 70  // octree stage: sorted indices and segment starts
#define DPF3_MAX_JOBS 65535 // clouds per launch of the kernels that take the cloud in blockIdx.y

struct Dpf3Preds {
    int n;
    sfe_icp_dpf s[SFE_DPF_MAX_STAGES];
};

// one workgroup per cloud: cloud c = src[src_off[c] .. + jobs[c].tot) -> dst[jobs[c].cat ..), jobs[c].tot = the kept points
// (L.n == 0: a copy into the working layout)
__global__ __launch_bounds__(DPF3_THREADS) void dpf3_predicate_kernel(Dpf3Preds L, const float *__restrict__ src,
                                                                      const long long *__restrict__ src_off,
                                                                      S3Job *__restrict__ jobs, float *__restrict__ dst)
{
    __shared__ int s_wave[DPF3_UNROLL][DPF3_THREADS / 64];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = jobs[c].tot;
    const float *p = src + 3 * (size_t)src_off[c];
    float *o = dst + 3 * (size_t)jobs[c].cat;
    __syncthreads(); // (every thread has read the size that thread 0 overwrites at the end)
    const unsigned long long below = (1ull << lane) - 1ull;
    int carry = 0;
    for (int base = 0; base < n; base += DPF3_THREADS * DPF3_UNROLL) {
        float q[DPF3_UNROLL][3];
        bool keep[DPF3_UNROLL];
#pragma unroll
        for (int u = 0; u < DPF3_UNROLL; ++u) {
            const int i = base + u * DPF3_THREADS + tid;
            keep[u] = i < n;
#pragma unroll
            for (int a = 0; a < 3; ++a)
                q[u][a] = keep[u] ? p[3 * (size_t)i + a] : 0.0f;
        }
        int at[DPF3_UNROLL];
#pragma unroll
        for (int u = 0; u < DPF3_UNROLL; ++u) {
            for (int s = 0; s < L.n; ++s)
                keep[u] = keep[u] && icp3_dpf_keep(L.s[s], q[u][0], q[u][1], q[u][2]);
            const unsigned long long m = __ballot(keep[u]);
            at[u] = __popcll(m & below);
            if (lane == 0)
                s_wave[u][wave] = __popcll(m);
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < DPF3_UNROLL; ++u) {
            int off = carry;
            for (int v = 0; v < u; ++v)
                for (int w = 0; w < DPF3_THREADS / 64; ++w)
                    off += s_wave[v][w];
            for (int w = 0; w < wave; ++w)
                off += s_wave[u][w];
            if (keep[u]) { // (off + at[u] < n: a kept point never moves behind its own index)
                float *d = o + 3 * (size_t)(off + at[u]);
                d[0] = q[u][0];
                d[1] = q[u][1];
                d[2] = q[u][2];
            }
        }
        for (int u = 0; u < DPF3_UNROLL; ++u)
            for (int w = 0; w < DPF3_THREADS / 64; ++w)
                carry += s_wave[u][w];
        __syncthreads();
    }
    if (tid == 0)
        jobs[c].tot = carry;
}

// behind an octree stage: a cloud's size is its leaf count
__global__ __launch_bounds__(256) void dpf3_take_leaves_kernel(S3Job *__restrict__ jobs, const S3Header *__restrict__ hdrs,
                                                               int n_clouds)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < n_clouds)
        jobs[c].tot = hdrs[c].n_seg;
}

static int dpf3_check_list(sfe_ctx *ctx, const sfe_icp_dpf *st, int n, const char *side)
{
    int bad = 0;
    switch (icp3_dpf_validate(st, n, &bad)) {
    case ICP3_DPF_OK:
        return 0;
    case ICP3_DPF_COUNT:
        return sfe_set_err(ctx, SFE_ERR_ARG, "3-D %s data-point filters: %d stages (0 to %d, with a stage array)", side, n,
                           SFE_DPF_MAX_STAGES);
    case ICP3_DPF_DIM:
        return sfe_set_err(ctx, SFE_ERR_ARG, "3-D %s data-point filter stage %d: dim %d is not -1, 0, 1 or 2", side, bad,
                           st[bad].dim);
    case ICP3_DPF_OCTREE_SIZE:
        return sfe_set_err(ctx, SFE_ERR_ARG, "3-D %s data-point filter stage %d: maxSizeByNode %g is not > 0", side, bad,
                           (double)st[bad].f[0]);
    default:
        return sfe_set_err(ctx, SFE_ERR_ARG, "3-D %s data-point filter stage %d: unknown kind %d", side, bad, st[bad].kind);
    }
}

int sfe_icp3_check_chain(sfe_ctx *ctx, const sfe_icp_outliers *o, const sfe_icp_dpf *rd, int n_rd, const sfe_icp_dpf *rf,
                         int n_rf)
{
    if (int rc = sfe_icp_check_outliers(ctx, o))
        return rc;
    if (int rc = dpf3_check_list(ctx, rd, n_rd, "reading"))
        return rc;
    return dpf3_check_list(ctx, rf, n_rf, "reference");
}

// The stages over n_clouds clouds: cloud c = d_in[in_start[c] .. + n[c]) -> d_out, back to back (room for the sum of n),
// kept counts to h_counts (host).  Enqueues everything, then synchronises once.
static int dpf3_run(sfe_ctx *ctx, const sfe_icp_dpf *st, int n_st, const float *d_in, const long long *in_start,
                    const int32_t *n, int n_clouds, float *d_out, int32_t *h_counts)
{
    const size_t nc = (size_t)n_clouds;
    std::vector<S3Job> jobs(nc);
    std::vector<long long> base(nc);
    long long total = 0;
    int max_n = 0;
    bool in_place = true; // the input already lies in the working layout
    for (size_t c = 0; c < nc; ++c) {
        if (n[c] < 0 || n[c] > S3_MAX_POINTS || in_start[c] < 0)
            return sfe_set_err(ctx, SFE_ERR_ARG, "3-D data-point filters: cloud %d has %d points at %lld", (int)c, n[c],
                               in_start[c]);
        base[c] = total;
        jobs[c] = S3Job{total, n[c], 0, 0, 0};
        in_place = in_place && in_start[c] == total;
        total += n[c];
        max_n = std::max(max_n, (int)n[c]);
    }
    // stage groups: a run of predicates, or one octree stage; a copy in front where an octree stage (or the placement)
    // would otherwise read an input that is not in the working layout
    std::vector<std::pair<int, int>> groups;
    for (int i = 0; i < n_st;) {
        int j = i + 1;
        if (st[i].kind != SFE_DPF_OCTREE_GRID)
            while (j < n_st && st[j].kind != SFE_DPF_OCTREE_GRID)
                ++j;
        groups.emplace_back(i, j);
        i = j;
    }
    if (!in_place && (groups.empty() || st[groups[0].first].kind == SFE_DPF_OCTREE_GRID))
        groups.insert(groups.begin(), std::make_pair(0, 0));
    bool has_octree = false;
    for (int i = 0; i < n_st; ++i)
        has_octree |= st[i].kind == SFE_DPF_OCTREE_GRID;

    const size_t np = (size_t)std::max(total, 1LL);
    // [jobs | in_start | base] go up; [off | hdr | cnt] stay on the device (cnt comes back)
    const size_t b_up = (sizeof(S3Job) + 16) * nc, b_tab = b_up + (8 + sizeof(S3Header) + 4) * nc;
    char *d_tab = (char *)sfe_scratch(ctx, DPF3_SLOT_TAB, b_tab);
    float *d_a = (float *)sfe_scratch(ctx, DPF3_SLOT_A, sizeof(float) * 3 * np);
    float *d_b = (float *)sfe_scratch(ctx, DPF3_SLOT_B, sizeof(float) * 3 * np);
    char *h_up = (char *)sfe_pinned_io(ctx, 0, b_up);
    int32_t *h_cnt = (int32_t *)sfe_pinned_io(ctx, 1, 4 * nc);
    if (!d_tab || !d_a || !d_b || !h_up || !h_cnt)
        return SFE_ERR_HIP;
    S3OctreeBufs ob{};
    if (has_octree) {
        ob.keys = (unsigned long long *)sfe_scratch(ctx, DPF3_SLOT_KEYS, 16 * np);
        ob.sidx = (int *)sfe_scratch(ctx, DPF3_SLOT_IDX, 4 * (2 * np + nc));
        if (!ob.keys || !ob.sidx)
            return SFE_ERR_HIP;
        ob.skeys = ob.keys + np;
        ob.seg = ob.sidx + np;
    }
    S3Job *d_jobs = (S3Job *)d_tab;
    long long *d_in_start = (long long *)(d_tab + sizeof(S3Job) * nc), *d_base = d_in_start + nc, *d_off = d_base + nc;
    S3Header *d_hdr = (S3Header *)(d_off + nc);
    int32_t *d_cnt = (int32_t *)(d_hdr + nc);
    memcpy(h_up, jobs.data(), sizeof(S3Job) * nc);
    memcpy(h_up + sizeof(S3Job) * nc, in_start, 8 * nc);
    memcpy(h_up + sizeof(S3Job) * nc + 8 * nc, base.data(), 8 * nc);
    SFE_HIP(ctx, hipMemcpyAsync(d_tab, h_up, b_up, hipMemcpyHostToDevice, ctx->stream));

    const float *cur = d_in;
    const long long *cur_off = d_in_start;
    for (size_t g = 0; g < groups.size(); ++g) {
        float *nxt = g & 1 ? d_b : d_a;
        const int i0 = groups[g].first, i1 = groups[g].second;
        if (i0 == i1 || st[i0].kind != SFE_DPF_OCTREE_GRID) {
            Dpf3Preds L{};
            L.n = i1 - i0;
            for (int i = i0; i < i1; ++i)
                L.s[i - i0] = st[i];
            hipLaunchKernelGGL(dpf3_predicate_kernel, dim3(n_clouds), dim3(DPF3_THREADS), 0, ctx->stream, L, cur, cur_off, d_jobs,
                               nxt);
        } else {
            const float max_size = sfe_s3_max_size(st[i0].f[0]);
            for (int first = 0; first < n_clouds; first += DPF3_MAX_JOBS) {
                S3OctreeBufs b = ob;
                b.hdr = d_hdr + first;
                b.out = nxt;
                if (int rc = sfe_s3_octree_enqueue(ctx, cur, d_jobs + first, std::min(DPF3_MAX_JOBS, n_clouds - first), max_n,
                                                   max_size, b))
                    return rc;
            }
            hipLaunchKernelGGL(dpf3_take_leaves_kernel, dim3((n_clouds + 255) / 256), dim3(256), 0, ctx->stream, d_jobs,
                               (const S3Header *)d_hdr, n_clouds);
        }
        SFE_LAUNCH_CHECK(ctx);
        cur = nxt;
        cur_off = d_base;
    }
    // back to back: cloud c after the survivors of the clouds in front of it
    if (int rc = sfe_s3_offsets_enqueue(ctx, d_jobs, d_hdr, n_clouds, 1, d_cnt, d_off))
        return rc;
    for (int first = 0; first < n_clouds; first += DPF3_MAX_JOBS)
        if (int rc = sfe_s3_place_enqueue(ctx, cur, d_jobs + first, std::min(DPF3_MAX_JOBS, n_clouds - first), max_n,
                                          d_cnt + first, d_off + first, 0, d_out))
            return rc;
    SFE_HIP(ctx, hipMemcpyAsync(h_cnt, d_cnt, 4 * nc, hipMemcpyDeviceToHost, ctx->stream));
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the pass's one synchronisation: the counts
    for (size_t c = 0; c < nc; ++c)
        if (h_cnt[c] < 0 || h_cnt[c] > n[c])
            return sfe_set_err(ctx, SFE_ERR_HIP, "3-D data-point filters: cloud %d left %d points of %d", (int)c, h_cnt[c], n[c]);
    memcpy(h_counts, h_cnt, 4 * nc);
    return 0;
}

// distinct (start, n) slices of a job table's source (col 0) or target (col 2) side, in first-use order
struct Dpf3Slices {
    std::vector<long long> start, base; // input offset, offset in the pool ICP runs on
    std::vector<int32_t> n, kept;
    std::vector<int> of_job;
};
static void dpf3_slices(const int64_t *jobs4, int n_jobs, int col, Dpf3Slices &s)
{
    std::map<std::pair<long long, int>, int> seen;
    s.of_job.resize((size_t)n_jobs);
    for (int j = 0; j < n_jobs; ++j) {
        const int64_t *q = jobs4 + 4 * (size_t)j + col;
        const auto key = std::make_pair((long long)q[0], (int)q[1]);
        auto it = seen.find(key);
        if (it == seen.end()) {
            it = seen.emplace(key, (int)s.n.size()).first;
            s.start.push_back(q[0]);
            s.n.push_back((int32_t)q[1]);
        }
        s.of_job[j] = it->second;
    }
}

int sfe_icp3_chain_run_dev(sfe_ctx *ctx, const sfe_icp_params *p, const sfe_icp_outliers *o, const sfe_icp_dpf *rd, int n_rd,
                           const sfe_icp_dpf *rf, int n_rf, const float *d_src, const float *d_tgt, const int64_t *jobs4,
                           const float *guesses16, int n_jobs, float *T_out16, int32_t *status, int32_t *iters)
{
    if (n_rd == 0 && n_rf == 0) // no stage: the plain launch on the caller's job table
        return sfe_icp3_run_dev(ctx, p, o, d_src, d_tgt, jobs4, guesses16, n_jobs, T_out16, status, iters);
    Dpf3Slices S, R;
    dpf3_slices(jobs4, n_jobs, 0, S);
    dpf3_slices(jobs4, n_jobs, 2, R);
    const float *fsrc = d_src, *ftgt = d_tgt;
    // (the filtered pools live in slots neither the filter pass of the other side nor the ICP launch touches)
    for (int side = 0; side < 2; ++side) {
        Dpf3Slices &D = side ? R : S;
        const sfe_icp_dpf *st = side ? rf : rd;
        const int n_st = side ? n_rf : n_rd;
        if (n_st == 0) {
            D.base = D.start;
            D.kept = D.n;
            continue;
        }
        long long total = 0;
        for (int32_t v : D.n)
            total += v;
        float *d_f = (float *)sfe_scratch(ctx, side ? DPF3_SLOT_TGT : DPF3_SLOT_SRC, sizeof(float) * 3 * (size_t)std::max(total, 1LL));
        if (!d_f)
            return SFE_ERR_HIP;
        D.kept.assign(D.n.size(), 0);
        if (int rc = dpf3_run(ctx, st, n_st, side ? d_tgt : d_src, D.start.data(), D.n.data(), (int)D.n.size(), d_f,
                              D.kept.data()))
            return rc;
        D.base.assign(D.n.size(), 0);
        long long at = 0;
        for (size_t c = 0; c < D.n.size(); ++c) {
            D.base[c] = at;
            at += D.kept[c];
        }
        (side ? ftgt : fsrc) = d_f;
    }
    // the ICP job table on the filtered pools; a job with an emptied cloud never reaches the kernel
    std::vector<int64_t> jobs;
    std::vector<int> idx;
    std::vector<float> g;
    for (int j = 0; j < n_jobs; ++j) {
        const int a = S.of_job[j], b = R.of_job[j];
        memcpy(T_out16 + 16 * (size_t)j, guesses16 + 16 * (size_t)j, sizeof(float) * 16);
        if (iters)
            iters[j] = 0;
        if (S.kept[a] == 0 || R.kept[b] == 0) {
            status[j] = SFE_ICP_DPF_EMPTY;
            continue;
        }
        idx.push_back(j);
        const int64_t q[4] = {S.base[a], S.kept[a], R.base[b], R.kept[b]};
        jobs.insert(jobs.end(), q, q + 4);
        g.insert(g.end(), guesses16 + 16 * (size_t)j, guesses16 + 16 * (size_t)j + 16);
    }
    const int m = (int)idx.size();
    if (m == 0)
        return 0;
    std::vector<float> T((size_t)m * 16);
    std::vector<int32_t> st((size_t)m * 2);
    if (int rc = sfe_icp3_run_dev(ctx, p, o, fsrc, ftgt, jobs.data(), g.data(), m, T.data(), st.data(), st.data() + m))
        return rc;
    for (int k = 0; k < m; ++k) {
        const int j = idx[k];
        memcpy(T_out16 + 16 * (size_t)j, T.data() + 16 * (size_t)k, sizeof(float) * 16);
        status[j] = st[k];
        if (iters)
            iters[j] = st[m + k];
    }
    return 0;
}

extern "C" {

int sfe_icp3_filter_clouds_dev(sfe_ctx *ctx, const sfe_icp_dpf *stages, int n_stages, const float *d_pts, const int64_t *off,
                               int n_clouds, float *d_out, int32_t *counts_out)
{
    if (int rc = sfe_use(ctx))
        return rc;
    SFE_ARG(ctx, n_clouds >= 0 && (n_clouds == 0 || (off && d_pts && d_out && counts_out)));
    if (int rc = dpf3_check_list(ctx, stages, n_stages, "cloud"))
        return rc;
    if (n_clouds == 0)
        return 0;
    std::vector<long long> in_start((size_t)n_clouds);
    std::vector<int32_t> n((size_t)n_clouds);
    for (int c = 0; c < n_clouds; ++c) {
        if (off[c] < 0 || off[c + 1] < off[c] || off[c + 1] - off[c] > S3_MAX_POINTS)
            return sfe_set_err(ctx, SFE_ERR_ARG, "sfe_icp3_filter_clouds_dev: off[%d..%d] = %lld, %lld", c, c + 1,
                               (long long)off[c], (long long)off[c + 1]);
        in_start[c] = off[c];
        n[c] = (int32_t)(off[c + 1] - off[c]);
    }
    return dpf3_run(ctx, stages, n_stages, d_pts, in_start.data(), n.data(), n_clouds, d_out, counts_out);
}

} // extern "C"
