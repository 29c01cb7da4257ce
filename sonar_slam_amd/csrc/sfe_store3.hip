// Device-resident keyframe clouds in 3-D: the keyframe store (sfe_store.hip) for N x 3 float32 clouds.
//
//   reference flow (host numpy; every keyframe's 3-D cloud is re-transformed at every graph update):
//     slam_objects.py:101-106   Keyframe.points3D / transf_points3D
//     slam_objects.py:200-223   Keyframe.transform_points_3D      points.dot(H[:3, :3].T) + H[:3, 3]   (float32)
//     slam.py:229-292           SLAM.get_points                   transform, concatenate, pcl.downsample
//     slam.py:294-323           SLAM.compute_icp                  pcl.ICP.compute(source, target, guess)
//     slam.py:389-424           SLAM.get_overlap                  transform, pcl.match, count ids != -1
//
//   here: one pool of packed float triples (12-byte stride, as in sfe_pcl3.hip) in HBM and a slot table {stamp, offset,
//   count} per cloud on the HOST (sfe_store3_slots.h).  Unlike the 2-D store no producer appends from device-side counts: a
//   cloud arrives from the host (put: its size is known) or from get_points (one synchronisation brings the sizes), so the
//   table needs no device copy and nothing can turn out not to fit after the fact.  Every kernel gets the offsets it needs in
//   a small per-call job table.  Clouds are named by handle (slot index); slots are released in stack order.
//
//   get_points   n_jobs targets per call, every stage ONE launch with the job in blockIdx.y (or .x for the one-workgroup
//                stages): transform + gather -> bounding box -> keys -> ranks -> segments -> medoids -> offsets -> place.
//                The downsample stages are the kernels of sfe_downsample3 (sfe_pcl3.hip: 8-way tree, rank-counting sort,
//                float centroid, first point at the minimum distance) with a job table in front, expression for expression,
//                so that a job's result is bit for bit pcl.downsample of its concatenation.  The results are placed one
//                behind the other at the pool's fill level (the offsets kernel scans the jobs' leaf counts on the device);
//                the host synchronises once, for the counts.
//   icp          icp3_job_kernel (sfe_icp3.hip) on the pool, its job table built from the slot table: no point is copied.
//   overlap      one lane per moved source point, the target tiled through LDS (2048 points), integer counts.
//
// The transform rule is numpy's for float32 arrays (sgemm, then the broadcast addition), per output coordinate i
//     fl( fma(p2, Hi2, fma(p1, Hi1, fl(p0 * Hi0))) + Hi3 )
// -- the 3-term form of SFE_STORE_F32_POINTS in sfe_store.hip -- written with explicit intrinsics.
#include "sfe_icp_common.h"
#include "sfe_store3_slots.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define S3_TILE 2048       // points per LDS tile (24 KiB), as P3_TILE of sfe_pcl3.hip
#define S3_MAX_LEVELS 21   // DS3_MAX_LEVELS
#define S3_MAX_POINTS (1 << 28) // largest cloud / concatenation: the kernels index a cloud's points with an int
#define S3_MAX_JOBS 65535  // blockIdx.y

struct sfe_cloud_store3 {
    sfe_ctx *ctx = nullptr;
    float *d_pool = nullptr; // [capacity][3]
    Store3Slots slots;
};

struct S3Seg { // one input cloud of a get_points job
    long long src; // its first point in the pool
    int n;         // its points (> 0: empty and unused entries are dropped on the host)
    int dst;       // its first point in the job's concatenation
    float H[12];   // rows 0..2 of the 4 x 4 transform
};

struct S3Job { // one get_points job
    long long cat; // first point of its concatenation in the scratch arrays
    int tot;       // points of the concatenation
    int seg0, nseg; // its segments
    int pad;
};

struct S3Header { // Ds3Header
    float cx, cy, cz, radius;
    int levels;
    int n_seg;
};

struct S3Pair { // one overlap job
    long long src, tgt; // first points in the pool
    int ns, nt;
    float H[12];
};

__device__ __forceinline__ float s3_dist2(float px, float py, float pz, float tx, float ty, float tz)
{
    const float dx = f_add(px, -tx), dy = f_add(py, -ty), dz = f_add(pz, -tz);
    return f_add(f_add(f_mul(dx, dx), f_mul(dy, dy)), f_mul(dz, dz));
}

// row i of the transform on a point: numpy's float32 `p.dot(R.T) + t`
__device__ __forceinline__ float s3_move(const float *row, float p0, float p1, float p2)
{
    return f_add(__fmaf_rn(p2, row[2], __fmaf_rn(p1, row[1], f_mul(p0, row[0]))), row[3]);
}

// ---------------------------------------------------------------------------------------------------------------------
// get_points
// ---------------------------------------------------------------------------------------------------------------------
// transform + gather: point i of job blockIdx.y's concatenation <- its cloud's point, moved
__global__ __launch_bounds__(256) void s3_gather_kernel(const float *__restrict__ pool, const S3Job *__restrict__ jobs,
                                                        const S3Seg *__restrict__ segs, float *__restrict__ cat)
{
    const S3Job J = jobs[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= J.tot)
        return;
    const S3Seg *sg = segs + J.seg0;
    int k = 0;
    while (k + 1 < J.nseg && i >= sg[k + 1].dst)
        ++k;
    const float *p = pool + 3 * (size_t)(sg[k].src + (i - sg[k].dst));
    const float p0 = p[0], p1 = p[1], p2 = p[2];
    float *o = cat + 3 * (size_t)(J.cat + i);
    o[0] = s3_move(sg[k].H, p0, p1, p2);
    o[1] = s3_move(sg[k].H + 4, p0, p1, p2);
    o[2] = s3_move(sg[k].H + 8, p0, p1, p2);
}

// ds3_bbox_kernel per job (one workgroup each): Octree::build's centre, radius and depth
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

// ds3_key_kernel per job
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

// ds3_rank_kernel per job: rank of (key_i, i) among the job's points = position in the stable sort
__global__ __launch_bounds__(256) void s3_rank_kernel(const unsigned long long *__restrict__ keys_all,
                                                      const S3Job *__restrict__ jobs, int *__restrict__ sorted_idx_all,
                                                      unsigned long long *__restrict__ sorted_key_all)
{
    __shared__ unsigned long long s_k[S3_TILE];
    const S3Job J = jobs[blockIdx.y];
    const int n = J.tot;
    if (blockIdx.x * 256 >= n) // (uniform: the whole workgroup leaves before any barrier)
        return;
    const unsigned long long *__restrict__ keys = keys_all + J.cat;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const unsigned long long ki = (i < n) ? keys[i] : 0ull;
    int rank = 0;
    for (int tb = 0; tb < n; tb += S3_TILE) {
        const int tn = min(S3_TILE, n - tb);
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

// ds3_segment_kernel per job (one workgroup each): the first position of every run of equal keys + a sentinel.  Job j's
// list has tot + 1 entries and begins at cat + j.
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

// ds3_medoid_kernel per job: one thread per leaf, float centroid in input order, the first point at the minimum distance
__global__ __launch_bounds__(256) void s3_medoid_kernel(const float *__restrict__ cat, const S3Job *__restrict__ jobs,
                                                        const int *__restrict__ sorted_idx_all,
                                                        const int *__restrict__ seg_start_all,
                                                        const S3Header *__restrict__ hdrs, float *__restrict__ out_all)
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
        const float d = sqrtf(s3_dist2(q[0], q[1], q[2], sx, sy, sz));
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

// ---------------------------------------------------------------------------------------------------------------------
// overlap: moved source points with a target point within the radius (the rules of match3_kernel)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void s3_overlap_kernel(const float *__restrict__ pool, const S3Pair *__restrict__ pairs,
                                                         float r2, int *__restrict__ counts)
{
    __shared__ float s_t[3 * S3_TILE];
    const S3Pair J = pairs[blockIdx.y];
    if (blockIdx.x * 256 >= J.ns) // (uniform)
        return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    float px = 0, py = 0, pz = 0;
    if (i < J.ns) {
        const float *p = pool + 3 * (size_t)(J.src + i);
        const float p0 = p[0], p1 = p[1], p2 = p[2];
        px = s3_move(J.H, p0, p1, p2);
        py = s3_move(J.H + 4, p0, p1, p2);
        pz = s3_move(J.H + 8, p0, p1, p2);
    }
    const float *__restrict__ tgt = pool + 3 * (size_t)J.tgt;
    bool hit = false;
    for (int tb = 0; tb < J.nt; tb += S3_TILE) {
        const int tn = min(S3_TILE, J.nt - tb);
        __syncthreads();
        for (int q = threadIdx.x; q < 3 * tn; q += 256) // consecutive floats: coalesced
            s_t[q] = tgt[3 * (size_t)tb + q];
        __syncthreads();
        for (int j = 0; j < tn; ++j) // every lane reads the same LDS words: a broadcast
            hit |= s3_dist2(px, py, pz, s_t[3 * j], s_t[3 * j + 1], s_t[3 * j + 2]) <= r2; // NaN: never
    }
    hit = hit && i < J.ns;
    const unsigned long long b = __ballot(hit);
    if ((threadIdx.x & 63) == 0 && b)
        atomicAdd(&counts[blockIdx.y], (int)__popcll(b));
}

// ---------------------------------------------------------------------------------------------------------------------
static int s3_check(sfe_ctx *ctx, sfe_cloud_store3 *s)
{
    if (int rc = sfe_use(ctx))
        return rc;
    SFE_ARG(ctx, s && s->ctx == ctx);
    return 0;
}

extern "C" {

int sfe_cloud_store3_create(sfe_ctx *ctx, int64_t capacity_points, int32_t max_clouds, sfe_cloud_store3 **out)
{
    if (int rc = sfe_use(ctx))
        return rc;
    SFE_ARG(ctx, out && capacity_points > 0 && capacity_points <= (1ll << 40) && max_clouds > 0);
    *out = nullptr;
    sfe_cloud_store3 *s = new sfe_cloud_store3();
    s->ctx = ctx;
    if (hipMalloc((void **)&s->d_pool, sizeof(float) * 3 * (size_t)capacity_points) != hipSuccess) {
        (void)hipGetLastError();
        delete s;
        return sfe_set_err(ctx, SFE_ERR_HIP, "3-D cloud store: allocating %lld points failed", (long long)capacity_points);
    }
    s->slots.init(capacity_points, max_clouds);
    *out = s;
    return 0;
}

void sfe_cloud_store3_destroy(sfe_cloud_store3 *s)
{
    if (!s)
        return;
    sfe_ctx *ctx = s->ctx;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(s->d_pool);
    delete s;
}

int sfe_cloud_store3_count(sfe_cloud_store3 *s) { return s ? s->slots.n_slots : 0; }

int sfe_cloud_store3_put(sfe_ctx *ctx, sfe_cloud_store3 *s, int64_t stamp, const float *pts, int n, int32_t *handle_out)
{
    if (int rc = s3_check(ctx, s))
        return rc;
    SFE_ARG(ctx, n >= 0 && n <= S3_MAX_POINTS && (n == 0 || pts) && handle_out);
    Store3Slots &t = s->slots;
    if (!t.fits(n, 1))
        return sfe_set_err(ctx, SFE_ERR_CAP, "3-D cloud store: a cloud of %d points does not fit (%lld of %lld points and %d of "
                                             "%d slots in use)", n, (long long)t.top, (long long)t.capacity, t.n_slots, t.max_clouds);
    if (n) {
        // through the event-guarded pinned staging: the caller's array may go away when the call returns
        const size_t bytes = sizeof(float) * 3 * (size_t)n;
        char *h = (char *)sfe_pinned_begin(ctx, bytes);
        if (!h)
            return SFE_ERR_HIP;
        memcpy(h, pts, bytes);
        SFE_HIP(ctx, hipMemcpyAsync(s->d_pool + 3 * (size_t)t.top, h, bytes, hipMemcpyHostToDevice, ctx->stream));
        if (int rc = sfe_pinned_end(ctx, ctx->stream))
            return rc;
    }
    *handle_out = t.push(stamp, n);
    return 0;
}

int sfe_cloud_store3_meta(sfe_ctx *ctx, sfe_cloud_store3 *s, int32_t first, int32_t n, int64_t *stamps, int64_t *offsets,
                          int32_t *counts)
{
    if (int rc = s3_check(ctx, s))
        return rc;
    SFE_ARG(ctx, first >= 0 && n >= 0 && (int64_t)first + n <= s->slots.n_slots);
    for (int i = 0; i < n; ++i) {
        if (stamps)
            stamps[i] = s->slots.stamp[(size_t)first + i];
        if (offsets)
            offsets[i] = s->slots.off[(size_t)first + i];
        if (counts)
            counts[i] = (int32_t)s->slots.cnt[(size_t)first + i];
    }
    return 0;
}

int sfe_cloud_store3_read(sfe_ctx *ctx, sfe_cloud_store3 *s, int32_t handle, float *out, int cap, int *n_out)
{
    if (int rc = s3_check(ctx, s))
        return rc;
    SFE_ARG(ctx, s->slots.valid(handle) && n_out && cap >= 0 && (cap == 0 || out));
    const int n = (int)s->slots.cnt[(size_t)handle];
    *n_out = n;
    if (n == 0)
        return 0;
    if (n > cap)
        return sfe_set_err(ctx, SFE_ERR_CAP, "3-D cloud store: cloud %d has %d points, the buffer holds %d", handle, n, cap);
    SFE_HIP(ctx, hipMemcpyAsync(out, s->d_pool + 3 * (size_t)s->slots.off[(size_t)handle], sizeof(float) * 3 * (size_t)n,
                                hipMemcpyDeviceToHost, ctx->stream));
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int sfe_cloud_store3_truncate(sfe_ctx *ctx, sfe_cloud_store3 *s, int32_t n_slots)
{
    if (int rc = s3_check(ctx, s))
        return rc;
    // (everything that reads the released clouds was enqueued on the context's stream before whatever overwrites them)
    SFE_ARG(ctx, s->slots.truncate(n_slots));
    return 0;
}

int sfe_cloud_store3_get_points(sfe_ctx *ctx, sfe_cloud_store3 *s, const int32_t *handles, const float *H12, int n_jobs, int m,
                                float resolution, const int64_t *stamps, int32_t *handles_out)
{
    if (int rc = s3_check(ctx, s))
        return rc;
    SFE_ARG(ctx, n_jobs >= 0 && n_jobs <= S3_MAX_JOBS && m >= 1 && (n_jobs == 0 || (handles && H12 && handles_out)));
    if (n_jobs == 0)
        return 0;
    Store3Slots &t = s->slots;
    std::vector<S3Job> jobs((size_t)n_jobs);
    std::vector<S3Seg> segs;
    int64_t total = 0;
    int max_tot = 0;
    for (int j = 0; j < n_jobs; ++j) {
        int64_t tot = 0;
        const int seg0 = (int)segs.size();
        for (int k = 0; k < m; ++k) {
            const size_t e = (size_t)j * m + k;
            const int h = handles[e];
            if (h == -1)
                continue;
            if (!t.valid(h))
                return sfe_set_err(ctx, SFE_ERR_ARG, "3-D get_points: job %d names cloud %d, the store holds %d", j, h, t.n_slots);
            if (t.cnt[(size_t)h] == 0)
                continue;
            S3Seg g;
            g.src = t.off[(size_t)h];
            g.n = (int)t.cnt[(size_t)h];
            g.dst = (int)tot;
            memcpy(g.H, H12 + 12 * e, sizeof g.H);
            tot += g.n;
            if (tot > S3_MAX_POINTS)
                return sfe_set_err(ctx, SFE_ERR_ARG, "3-D get_points: job %d concatenates more than %d points", j, S3_MAX_POINTS);
            segs.push_back(g);
        }
        jobs[(size_t)j] = {total, (int)tot, seg0, (int)segs.size() - seg0, 0};
        total += tot;
        max_tot = std::max(max_tot, (int)tot);
    }
    // the call's upper bound: no downsample leaves more points than it was given
    if (!t.fits(total, n_jobs))
        return sfe_set_err(ctx, SFE_ERR_CAP, "3-D get_points: %d clouds of up to %lld points in all do not fit (%lld of %lld points "
                                             "and %d of %d slots in use)", n_jobs, (long long)total, (long long)t.top,
                           (long long)t.capacity, t.n_slots, t.max_clouds);
    const int raw = !(resolution > 0.0f);
    char buf[64];
    snprintf(buf, sizeof buf, "%f", (double)resolution); // pcl.cpp:134: std::to_string(float), as sfe_downsample3
    const float max_size = strtof(buf, nullptr);

    const size_t np = (size_t)std::max<int64_t>(total, 1);
    const size_t b_jobs = sizeof(S3Job) * (size_t)n_jobs, b_segs = sizeof(S3Seg) * segs.size(), b_tab = b_jobs + b_segs;
    const size_t b_cnt = sizeof(int32_t) * (size_t)n_jobs;
    char *h_tab = (char *)sfe_pinned_io(ctx, 2, b_tab);
    int32_t *h_cnt = (int32_t *)sfe_pinned_io(ctx, 3, b_cnt);
    float *d_cat = (float *)sfe_scratch(ctx, 0, sizeof(float) * 3 * np);
    unsigned long long *d_keys = (unsigned long long *)sfe_scratch(ctx, 1, 8 * np);
    unsigned long long *d_skeys = (unsigned long long *)sfe_scratch(ctx, 2, 8 * np);
    int *d_sidx = (int *)sfe_scratch(ctx, 3, 4 * np);
    int *d_seg = (int *)sfe_scratch(ctx, 4, 4 * (np + (size_t)n_jobs));
    float *d_out = (float *)sfe_scratch(ctx, 5, sizeof(float) * 3 * np);
    char *d_tab = (char *)sfe_scratch(ctx, 6, b_tab);
    S3Header *d_hdr = (S3Header *)sfe_scratch(ctx, 7, sizeof(S3Header) * (size_t)n_jobs);
    char *d_place = (char *)sfe_scratch(ctx, 8, (sizeof(long long) + sizeof(int32_t)) * (size_t)n_jobs);
    if (!h_tab || !h_cnt || !d_cat || !d_keys || !d_skeys || !d_sidx || !d_seg || !d_out || !d_tab || !d_hdr || !d_place)
        return SFE_ERR_HIP;
    memcpy(h_tab, jobs.data(), b_jobs);
    if (b_segs)
        memcpy(h_tab + b_jobs, segs.data(), b_segs);
    SFE_HIP(ctx, hipMemcpyAsync(d_tab, h_tab, b_tab, hipMemcpyHostToDevice, ctx->stream));
    const S3Job *d_jobs = (const S3Job *)d_tab;
    const S3Seg *d_segs = (const S3Seg *)(d_tab + b_jobs);
    long long *d_off = (long long *)d_place;
    int32_t *d_cnt = (int32_t *)(d_place + sizeof(long long) * (size_t)n_jobs);
    const unsigned nb = (unsigned)std::max((max_tot + 255) / 256, 1);
    const dim3 per_point(nb, (unsigned)n_jobs), per_job((unsigned)n_jobs);
    hipLaunchKernelGGL(s3_gather_kernel, per_point, dim3(256), 0, ctx->stream, (const float *)s->d_pool, d_jobs, d_segs, d_cat);
    if (!raw) {
        hipLaunchKernelGGL(s3_bbox_kernel, per_job, dim3(1024), 0, ctx->stream, (const float *)d_cat, d_jobs, max_size, d_hdr);
        hipLaunchKernelGGL(s3_key_kernel, per_point, dim3(256), 0, ctx->stream, (const float *)d_cat, d_jobs,
                           (const S3Header *)d_hdr, d_keys);
        hipLaunchKernelGGL(s3_rank_kernel, per_point, dim3(256), 0, ctx->stream, (const unsigned long long *)d_keys, d_jobs, d_sidx,
                           d_skeys);
        hipLaunchKernelGGL(s3_segment_kernel, per_job, dim3(1024), 0, ctx->stream, (const unsigned long long *)d_skeys, d_jobs,
                           d_seg, d_hdr);
        hipLaunchKernelGGL(s3_medoid_kernel, per_point, dim3(256), 0, ctx->stream, (const float *)d_cat, d_jobs,
                           (const int *)d_sidx, (const int *)d_seg, (const S3Header *)d_hdr, d_out);
    }
    hipLaunchKernelGGL(s3_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, d_jobs, (const S3Header *)d_hdr, n_jobs, raw, d_cnt,
                       d_off);
    // (the results lie within [top, top + total): the sum of the jobs' sizes is at most the bound tested above)
    hipLaunchKernelGGL(s3_place_kernel, dim3(std::min(3u * nb, 64u), (unsigned)n_jobs), dim3(256), 0, ctx->stream,
                       (const float *)(raw ? d_cat : d_out), d_jobs, (const int *)d_cnt, (const long long *)d_off,
                       (long long)t.top, s->d_pool);
    SFE_LAUNCH_CHECK(ctx);
    SFE_HIP(ctx, hipMemcpyAsync(h_cnt, d_cnt, b_cnt, hipMemcpyDeviceToHost, ctx->stream));
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the call's one synchronisation: the sizes
    for (int j = 0; j < n_jobs; ++j)
        if (h_cnt[j] < 0 || h_cnt[j] > jobs[(size_t)j].tot || (jobs[(size_t)j].tot > 0 && h_cnt[j] == 0))
            return sfe_set_err(ctx, SFE_ERR_HIP, "3-D get_points: job %d left %d points of %d", j, h_cnt[j], jobs[(size_t)j].tot);
    for (int j = 0; j < n_jobs; ++j)
        handles_out[j] = t.push(stamps ? stamps[j] : 0, h_cnt[j]);
    return 0;
}

int sfe_icp3_store_compute(sfe_ctx *ctx, const sfe_icp_params *p, sfe_cloud_store3 *s, const int32_t *pairs,
                           const float *guesses16, int n_jobs, float *T_out16, int32_t *status, int32_t *iters)
{
    if (int rc = s3_check(ctx, s))
        return rc;
    if (int rc = sfe_icp3_check_params(ctx, p))
        return rc;
    SFE_ARG(ctx, n_jobs >= 0 && (n_jobs == 0 || (pairs && guesses16 && T_out16 && status)));
    if (n_jobs == 0)
        return 0;
    const Store3Slots &t = s->slots;
    std::vector<int64_t> jobs4(4 * (size_t)n_jobs);
    for (int j = 0; j < n_jobs; ++j) {
        const int hs = pairs[2 * j], ht = pairs[2 * j + 1];
        if (!t.valid(hs) || !t.valid(ht))
            return sfe_set_err(ctx, SFE_ERR_ARG, "3-D scan match %d names clouds (%d, %d), the store holds %d", j, hs, ht, t.n_slots);
        if (t.cnt[(size_t)hs] <= 0 || t.cnt[(size_t)ht] <= 0)
            return sfe_set_err(ctx, SFE_ERR_ARG, "3-D scan match %d: cloud %d has %lld points, cloud %d has %lld (ICP needs "
                                                 "non-empty clouds)", j, hs, (long long)t.cnt[(size_t)hs], ht,
                               (long long)t.cnt[(size_t)ht]);
        jobs4[4 * (size_t)j] = t.off[(size_t)hs];
        jobs4[4 * (size_t)j + 1] = t.cnt[(size_t)hs];
        jobs4[4 * (size_t)j + 2] = t.off[(size_t)ht];
        jobs4[4 * (size_t)j + 3] = t.cnt[(size_t)ht];
    }
    return sfe_icp3_run_dev(ctx, p, s->d_pool, s->d_pool, jobs4.data(), guesses16, n_jobs, T_out16, status, iters);
}

int sfe_cloud_store3_overlap(sfe_ctx *ctx, sfe_cloud_store3 *s, const int32_t *pairs, const float *H12, int n_jobs,
                             float max_dist, int32_t *counts_out)
{
    if (int rc = s3_check(ctx, s))
        return rc;
    SFE_ARG(ctx, n_jobs >= 0 && n_jobs <= S3_MAX_JOBS && (n_jobs == 0 || (pairs && H12 && counts_out)));
    if (n_jobs == 0)
        return 0;
    const Store3Slots &t = s->slots;
    const size_t b_in = sizeof(S3Pair) * (size_t)n_jobs, b_out = sizeof(int32_t) * (size_t)n_jobs;
    S3Pair *h_in = (S3Pair *)sfe_pinned_io(ctx, 2, b_in);
    int32_t *h_out = (int32_t *)sfe_pinned_io(ctx, 3, b_out);
    S3Pair *d_in = (S3Pair *)sfe_scratch(ctx, 6, b_in);
    int32_t *d_out = (int32_t *)sfe_scratch(ctx, 7, b_out);
    if (!h_in || !h_out || !d_in || !d_out)
        return SFE_ERR_HIP;
    int max_ns = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const int hs = pairs[2 * j], ht = pairs[2 * j + 1];
        if (!t.valid(hs) || !t.valid(ht))
            return sfe_set_err(ctx, SFE_ERR_ARG, "3-D overlap %d names clouds (%d, %d), the store holds %d", j, hs, ht, t.n_slots);
        S3Pair &q = h_in[j];
        q.src = t.off[(size_t)hs];
        q.tgt = t.off[(size_t)ht];
        q.ns = (int)t.cnt[(size_t)hs];
        q.nt = (int)t.cnt[(size_t)ht];
        memcpy(q.H, H12 + 12 * (size_t)j, sizeof q.H);
        max_ns = std::max(max_ns, q.ns);
    }
    // match3_kernel takes a target only if its distance is below +inf, then tests it against the radius: one comparison
    // against min(r2, FLT_MAX) (a NaN radius stays NaN: nothing matches)
    float r2 = max_dist * max_dist; // as sfe_match forms it
    if (r2 > FLT_MAX)
        r2 = FLT_MAX;
    SFE_HIP(ctx, hipMemcpyAsync(d_in, h_in, b_in, hipMemcpyHostToDevice, ctx->stream));
    SFE_HIP(ctx, hipMemsetAsync(d_out, 0, b_out, ctx->stream));
    hipLaunchKernelGGL(s3_overlap_kernel, dim3((unsigned)std::max((max_ns + 255) / 256, 1), (unsigned)n_jobs), dim3(256), 0,
                       ctx->stream, (const float *)s->d_pool, (const S3Pair *)d_in, r2, d_out);
    SFE_LAUNCH_CHECK(ctx);
    SFE_HIP(ctx, hipMemcpyAsync(h_out, d_out, b_out, hipMemcpyDeviceToHost, ctx->stream));
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(counts_out, h_out, b_out);
    return 0;
}

} // extern "C"
