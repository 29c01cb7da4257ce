// pcl.downsample on N x 3 clouds (pcl.cpp:128-174), many clouds per launch: the rank-counting chain of sfe_downsample.hip on
// libpointmatcher's 8-way tree -- child bit0 = x > cx, bit1 = y > cy, bit2 = z > cz, 3 key bits per level, at most 21 levels
// in a 64-bit key (the 2-D chain: 2 bits, 31 levels); a deeper tree is cut at the cap.  bounding box -> keys -> rank-counting
// sort -> segments -> medoids (float centroid in input order, first point at the minimum distance), then the offsets and the
// placement of the jobs' results one behind the other.  Every stage is ONE launch with the job in blockIdx.y (or .x for the
// one-workgroup stages) and the job's offsets in a small table (S3Job, sfe_store3_slots.h); a job's result is bit for bit
// pcl.downsample of its cloud.  sfe_octree3.h names the callers; a single cloud is a one-job launch.
#include "sfe_octree3.h"
#include "sfe_points3.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

// one workgroup per job: Octree::build's centre, radius and depth
__global__ __launch_bounds__(1024) void s3_bbox_kernel(const float *__restrict__ cat, const S3Job *__restrict__ jobs,
                                                       float max_size, S3Header *__restrict__ hdrs)
{
    __shared__ float s_mn[3][16], s_mx[3][16];
    const S3Job J = jobs[blockIdx.x];
    const int n = J.tot;
    const float *__restrict__ pts = cat + 3 * (size_t)J.cat;
    S3Header *hdr = hdrs + blockIdx.x;
    if (n == 0) { // (uniform) an empty job: no leaf
        if (threadIdx.x == 0) {
            hdr->cx = hdr->cy = hdr->cz = hdr->radius = 0.0f;
            hdr->levels = 0;
            hdr->n_seg = 0;
        }
        return;
    }
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = threadIdx.x; i < n; i += 1024) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = pts[3 * (size_t)i + a];
            mn[a] = fminf(mn[a], v);
            mx[a] = fmaxf(mx[a], v);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            mn[a] = fminf(mn[a], __shfl_down(mn[a], d));
            mx[a] = fmaxf(mx[a], __shfl_down(mx[a], d));
        }
        if ((threadIdx.x & 63) == 0) {
            s_mn[a][threadIdx.x >> 6] = mn[a];
            s_mx[a][threadIdx.x >> 6] = mx[a];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float c[3], radius = 0.0f;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            for (int w = 1; w < 16; ++w) {
                mn[a] = fminf(mn[a], s_mn[a][w]);
                mx[a] = fmaxf(mx[a], s_mx[a][w]);
            }
            // Octree::build: centre = min + radii*0.5, radius = max(radii)*0.5
            const float ext = mx[a] - mn[a];
            c[a] = mn[a] + ext * 0.5f;
            if (a == 0 || radius < ext)
                radius = ext;
        }
        radius *= 0.5f;
        hdr->cx = c[0];
        hdr->cy = c[1];
        hdr->cz = c[2];
        hdr->radius = radius;
        int L = 0;
        float r = radius;
        while (!((double)r * 2.0 <= (double)max_size) && L < S3_MAX_LEVELS) {
            r *= 0.5f;
            ++L;
        }
        hdr->levels = L;
        hdr->n_seg = 0;
    }
}

// one lane per point: its path down the job's tree
__global__ __launch_bounds__(256) void s3_key_kernel(const float *__restrict__ cat, const S3Job *__restrict__ jobs,
                                                     const S3Header *__restrict__ hdrs, unsigned long long *__restrict__ keys)
{
    const S3Job J = jobs[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= J.tot)
        return;
    const float *q = cat + 3 * (size_t)(J.cat + i);
    const float px = q[0], py = q[1], pz = q[2];
    const S3Header *hdr = hdrs + blockIdx.y;
    float cx = hdr->cx, cy = hdr->cy, cz = hdr->cz, r = hdr->radius;
    const int L = hdr->levels;
    unsigned long long key = 0;
    for (int l = 0; l < L; ++l) {
        const unsigned bx = px > cx, by = py > cy, bz = pz > cz; // Octree::idx: bit i = pt(i) > centre(i)
        key = (key << 3) | (bx | (by << 1) | (bz << 2));
        const float hr = r * 0.5f;
        cx = cx + (bx ? hr : -hr);
        cy = cy + (by ? hr : -hr);
        cz = cz + (bz ? hr : -hr);
        r = hr;
    }
    keys[J.cat + i] = key;
}

// rank of (key_i, i) among the job's points = position in the stable sort; scatter index and key there
__global__ __launch_bounds__(256) void s3_rank_kernel(const unsigned long long *__restrict__ keys_all,
                                                      const S3Job *__restrict__ jobs, int *__restrict__ sorted_idx_all,
                                                      unsigned long long *__restrict__ sorted_key_all)
{
    __shared__ unsigned long long s_k[P3_TILE];
    const S3Job J = jobs[blockIdx.y];
    const int n = J.tot;
    if (blockIdx.x * 256 >= n) // (uniform: the whole workgroup leaves before any barrier)
        return;
    const unsigned long long *__restrict__ keys = keys_all + J.cat;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const unsigned long long ki = (i < n) ? keys[i] : 0ull;
    int rank = 0;
    for (int tb = 0; tb < n; tb += P3_TILE) {
        const int tn = min(P3_TILE, n - tb);
        __syncthreads();
        for (int q = threadIdx.x; q < tn; q += 256)
            s_k[q] = keys[tb + q];
        __syncthreads();
        for (int q = 0; q < tn; ++q) {
            const unsigned long long kj = s_k[q];
            rank += (kj < ki) || (kj == ki && tb + q < i);
        }
    }
    if (i < n) { // (rank < n: it counts points other than i)
        sorted_idx_all[J.cat + rank] = i;
        sorted_key_all[J.cat + rank] = ki;
    }
}

// one workgroup per job: the first position of every run of equal keys, listed in order, + a sentinel.  Job j's list has
// tot + 1 entries and begins at cat + j.
__global__ __launch_bounds__(1024) void s3_segment_kernel(const unsigned long long *__restrict__ sorted_key_all,
                                                          const S3Job *__restrict__ jobs, int *__restrict__ seg_start_all,
                                                          S3Header *__restrict__ hdrs)
{
    __shared__ int s_part[1024];
    const S3Job J = jobs[blockIdx.x];
    const int n = J.tot;
    const unsigned long long *__restrict__ sorted_key = sorted_key_all + J.cat;
    int *__restrict__ seg_start = seg_start_all + J.cat + blockIdx.x;
    const int per = (n + 1023) / 1024;
    const int b = (int)min((long long)threadIdx.x * per, (long long)n), e = min(b + per, n);
    int c = 0;
    for (int r = b; r < e; ++r)
        c += (r == 0) || (sorted_key[r] != sorted_key[r - 1]);
    s_part[threadIdx.x] = c;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int v = (threadIdx.x >= d) ? s_part[threadIdx.x - d] : 0;
        __syncthreads();
        s_part[threadIdx.x] += v;
        __syncthreads();
    }
    int s = (threadIdx.x == 0) ? 0 : s_part[threadIdx.x - 1];
    for (int r = b; r < e; ++r)
        if ((r == 0) || (sorted_key[r] != sorted_key[r - 1]))
            seg_start[s++] = r;
    if (threadIdx.x == 1023) {
        hdrs[blockIdx.x].n_seg = s_part[1023];
        seg_start[s_part[1023]] = n; // sentinel (n_seg <= n)
    }
}

// one thread per leaf: float centroid in input order, the first point at the minimum distance from it;
// IDX: the medoid's index in the job's concatenation goes to out_idx_all (the index output of sfe_downsample3)
template <bool IDX>
__global__ __launch_bounds__(256) void s3_medoid_kernel(const float *__restrict__ cat, const S3Job *__restrict__ jobs,
                                                        const int *__restrict__ sorted_idx_all,
                                                        const int *__restrict__ seg_start_all,
                                                        const S3Header *__restrict__ hdrs, float *__restrict__ out_all,
                                                        int *__restrict__ out_idx_all)
{
    const S3Job J = jobs[blockIdx.y];
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= hdrs[blockIdx.y].n_seg)
        return;
    const float *__restrict__ pts = cat + 3 * (size_t)J.cat;
    const int *__restrict__ sorted_idx = sorted_idx_all + J.cat;
    const int *__restrict__ seg_start = seg_start_all + J.cat + blockIdx.y;
    const int r0 = seg_start[s], r1 = seg_start[s + 1];
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (int r = r0; r < r1; ++r) {
        const float *q = pts + 3 * (size_t)sorted_idx[r];
        sx = f_add(sx, q[0]);
        sy = f_add(sy, q[1]);
        sz = f_add(sz, q[2]);
    }
    const float cnt = (float)(r1 - r0);
    sx = __fdiv_rn(sx, cnt);
    sy = __fdiv_rn(sy, cnt);
    sz = __fdiv_rn(sz, cnt);
    float best = 3.402823466e+38f;
    int bi = sorted_idx[r0];
    for (int r = r0; r < r1; ++r) {
        const int id = sorted_idx[r];
        const float *q = pts + 3 * (size_t)id;
        // sqrtf: the correctly rounded sequence (ds_medoid_kernel says why)
        const float d = sqrtf(p3_dist2(q[0], q[1], q[2], sx, sy, sz));
        if (d < best) {
            best = d;
            bi = id;
        }
    }
    const float *q = pts + 3 * (size_t)bi;
    float *o = out_all + 3 * (size_t)(J.cat + s);
    o[0] = q[0];
    o[1] = q[1];
    o[2] = q[2];
    if (IDX)
        out_idx_all[J.cat + s] = bi;
}

// one workgroup: every job's output size (its leaves, or with `raw` its whole concatenation) and the exclusive sum of the
// sizes in front of it = its place behind the pool's fill level
__global__ __launch_bounds__(1024) void s3_offsets_kernel(const S3Job *__restrict__ jobs, const S3Header *__restrict__ hdrs,
                                                          int n_jobs, int raw, int *__restrict__ out_cnt,
                                                          long long *__restrict__ out_off)
{
    __shared__ long long s_part[1024];
    const int per = (n_jobs + 1023) / 1024;
    const int b = min((int)threadIdx.x * per, n_jobs), e = min(b + per, n_jobs);
    long long c = 0;
    for (int j = b; j < e; ++j)
        c += raw ? jobs[j].tot : hdrs[j].n_seg;
    s_part[threadIdx.x] = c;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const long long v = (threadIdx.x >= d) ? s_part[threadIdx.x - d] : 0;
        __syncthreads();
        s_part[threadIdx.x] += v;
        __syncthreads();
    }
    long long at = (threadIdx.x == 0) ? 0 : s_part[threadIdx.x - 1];
    for (int j = b; j < e; ++j) {
        const int cj = raw ? jobs[j].tot : hdrs[j].n_seg;
        out_cnt[j] = cj;
        out_off[j] = at;
        at += cj;
    }
}

// the jobs' results, one behind the other, into the pool at `top` (in points)
__global__ __launch_bounds__(256) void s3_place_kernel(const float *__restrict__ from, const S3Job *__restrict__ jobs,
                                                       const int *__restrict__ out_cnt, const long long *__restrict__ out_off,
                                                       long long top, float *__restrict__ pool)
{
    const S3Job J = jobs[blockIdx.y];
    const long long nf = 3ll * out_cnt[blockIdx.y]; // (<= 3 tot)
    const float *__restrict__ src = from + 3 * (size_t)J.cat;
    float *__restrict__ dst = pool + 3 * (size_t)(top + out_off[blockIdx.y]);
    for (long long f = blockIdx.x * 256ll + threadIdx.x; f < nf; f += 256ll * gridDim.x)
        dst[f] = src[f];
}

float sfe_s3_max_size(float resolution)
{
    char buf[64];
    snprintf(buf, sizeof buf, "%f", (double)resolution); // pcl.cpp:134: std::to_string(float)
    return strtof(buf, nullptr);
}

int sfe_s3_octree_enqueue(sfe_ctx *ctx, const float *d_cat, const S3Job *d_jobs, int n_jobs, int max_tot, float max_size,
                          const S3OctreeBufs &b)
{
    SFE_ARG(ctx, n_jobs >= 1 && n_jobs <= S3_MAX_JOBS && max_tot >= 0);
    const unsigned nb = (unsigned)std::max((max_tot + 255) / 256, 1);
    const dim3 per_point(nb, (unsigned)n_jobs), per_job((unsigned)n_jobs);
    hipLaunchKernelGGL(s3_bbox_kernel, per_job, dim3(1024), 0, ctx->stream, d_cat, d_jobs, max_size, b.hdr);
    hipLaunchKernelGGL(s3_key_kernel, per_point, dim3(256), 0, ctx->stream, d_cat, d_jobs, (const S3Header *)b.hdr, b.keys);
    hipLaunchKernelGGL(s3_rank_kernel, per_point, dim3(256), 0, ctx->stream, (const unsigned long long *)b.keys, d_jobs, b.sidx,
                       b.skeys);
    hipLaunchKernelGGL(s3_segment_kernel, per_job, dim3(1024), 0, ctx->stream, (const unsigned long long *)b.skeys, d_jobs, b.seg,
                       b.hdr);
    if (b.midx)
        hipLaunchKernelGGL(s3_medoid_kernel<true>, per_point, dim3(256), 0, ctx->stream, d_cat, d_jobs, (const int *)b.sidx,
                           (const int *)b.seg, (const S3Header *)b.hdr, b.out, b.midx);
    else
        hipLaunchKernelGGL(s3_medoid_kernel<false>, per_point, dim3(256), 0, ctx->stream, d_cat, d_jobs, (const int *)b.sidx,
                           (const int *)b.seg, (const S3Header *)b.hdr, b.out, (int *)nullptr);
    SFE_LAUNCH_CHECK(ctx);
    return 0;
}

int sfe_s3_offsets_enqueue(sfe_ctx *ctx, const S3Job *d_jobs, const S3Header *d_hdr, int n_jobs, int raw, int *d_cnt,
                           long long *d_off)
{
    hipLaunchKernelGGL(s3_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, d_jobs, d_hdr, n_jobs, raw, d_cnt, d_off);
    SFE_LAUNCH_CHECK(ctx);
    return 0;
}

int sfe_s3_place_enqueue(sfe_ctx *ctx, const float *d_from, const S3Job *d_jobs, int n_jobs, int max_tot, const int *d_cnt,
                         const long long *d_off, long long top, float *pool)
{
    SFE_ARG(ctx, n_jobs >= 1 && n_jobs <= S3_MAX_JOBS && max_tot >= 0);
    const unsigned nb = (unsigned)std::max((max_tot + 255) / 256, 1);
    hipLaunchKernelGGL(s3_place_kernel, dim3(std::min(3u * nb, 64u), (unsigned)n_jobs), dim3(256), 0, ctx->stream, d_from, d_jobs,
                       d_cnt, d_off, top, pool);
    SFE_LAUNCH_CHECK(ctx);
    return 0;
}
