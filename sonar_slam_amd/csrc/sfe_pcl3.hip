// The cloud functions of bruce_slam.pcl on N x 3 clouds: match, remove_outlier, knn_density and downsample
// (pcl.cpp:54-74, 76-88, 128-174 are dimension-generic: fromEigen labels a z row when mat.cols() == 3 and every function
// returns topRows(mat_in.cols())).  The reference carries such clouds (Keyframe.points3D, slam_objects.py:101-106).
//
// These are the 3-D counterparts of match_kernel / match_knn_kernel / knn_density_kernel / radius_count_kernel
// (sfe_icp.hip) and of the rank-counting downsample chain (sfe_downsample.hip), written as kernels of their own: the 2-D
// kernels and their launchers are untouched.  The rules are the 2-D rules with one more coordinate:
//   d2 = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)), no fma; a z of 0 on both sides adds +0 and leaves the 2-D value;
//   the octree is 8-way: child bit0 = x > cx, bit1 = y > cy, bit2 = z > cz, 3 key bits per level, at most 21 levels in
//   a 64-bit key (the 2-D chain: 2 bits, 31 levels); a deeper tree is cut at the cap.
// Points are packed float triples (12-byte stride, a contiguous N x 3 float32 array): no padding is asked of the caller,
// and nothing is read as float4.  The reference cloud / the point tile goes through LDS, 2048 points (24 KiB) at a time;
// all lanes read the same LDS word in the inner loop (a broadcast).  Every kernel is brute force and quadratic in the
// cloud size, like its 2-D counterpart.
#include "sfe_icp_common.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#define P3_TILE 2048
#define DS3_MAX_LEVELS 21

struct Ds3Header {
    float cx, cy, cz, radius;
    int levels;
    int n_seg;
};

__device__ __forceinline__ float dist2_3(float px, float py, float pz, float tx, float ty, float tz)
{
    const float dx = f_add(px, -tx), dy = f_add(py, -ty), dz = f_add(pz, -tz);
    return f_add(f_add(f_mul(dx, dx), f_mul(dy, dy)), f_mul(dz, dz));
}

// points [tb, tb + tn) of a packed cloud -> s[0 .. 3 tn), by all 256 threads (consecutive floats: coalesced)
__device__ __forceinline__ void p3_stage(float *s, const float *__restrict__ pts, int tb, int tn)
{
    const float *src = pts + 3 * (size_t)tb;
    for (int j = threadIdx.x; j < 3 * tn; j += 256)
        s[j] = src[j];
}

// pcl.match, knn = 1: one lane per query, the reference tiled through LDS; ties -> the lowest reference index
__global__ __launch_bounds__(256) void match3_kernel(const float *__restrict__ ref, int nref, const float *__restrict__ in,
                                                     int nin, float r2, int *__restrict__ ids, float *__restrict__ d2)
{
    __shared__ float s_ref[3 * P3_TILE];
    const int i = blockIdx.x * 256 + threadIdx.x;
    float px = 0, py = 0, pz = 0;
    if (i < nin) {
        px = in[3 * (size_t)i];
        py = in[3 * (size_t)i + 1];
        pz = in[3 * (size_t)i + 2];
    }
    float best = INFINITY;
    int bi = -1;
    for (int tb = 0; tb < nref; tb += P3_TILE) {
        const int tn = min(P3_TILE, nref - tb);
        __syncthreads();
        p3_stage(s_ref, ref, tb, tn);
        __syncthreads();
        for (int j = 0; j < tn; ++j) {
            const float d = dist2_3(px, py, pz, s_ref[3 * j], s_ref[3 * j + 1], s_ref[3 * j + 2]);
            if (d < best) {
                best = d;
                bi = tb + j;
            }
        }
    }
    if (i < nin) {
        if (bi < 0 || !(best <= r2)) {
            bi = -1;
            best = INFINITY;
        }
        ids[i] = bi;
        d2[i] = best;
    }
}

// knn > 1: neighbour j is the lexicographic minimum of (d2, index) above neighbour j - 1, one pass over the reference
// per neighbour (match_knn_kernel's scheme); -1 / inf from the first neighbour beyond the radius on
__global__ __launch_bounds__(256) void match_knn3_kernel(const float *__restrict__ ref, int nref,
                                                         const float *__restrict__ in, int nin, int knn, float r2,
                                                         int *__restrict__ ids, float *__restrict__ d2)
{
    __shared__ float s_ref[3 * P3_TILE];
    const int i = blockIdx.x * 256 + threadIdx.x;
    float px = 0, py = 0, pz = 0;
    if (i < nin) {
        px = in[3 * (size_t)i];
        py = in[3 * (size_t)i + 1];
        pz = in[3 * (size_t)i + 2];
    }
    float prev_d = -1.0f; // every distance is >= 0
    int prev_i = -1;
    for (int jn = 0; jn < knn; ++jn) {
        float best = INFINITY;
        int bi = -1;
        for (int tb = 0; tb < nref; tb += P3_TILE) {
            const int tn = min(P3_TILE, nref - tb);
            __syncthreads();
            p3_stage(s_ref, ref, tb, tn);
            __syncthreads();
            for (int j = 0; j < tn; ++j) {
                const float d = dist2_3(px, py, pz, s_ref[3 * j], s_ref[3 * j + 1], s_ref[3 * j + 2]);
                const bool after = d > prev_d || (d == prev_d && tb + j > prev_i); // NaN: never
                if (after && d < best) { // ascending index: the first point attaining the minimum wins
                    best = d;
                    bi = tb + j;
                }
            }
        }
        if (bi < 0 || !(best <= r2)) {
            bi = -1;
            best = INFINITY;
        }
        if (i < nin) {
            ids[(size_t)jn * nin + i] = bi;
            d2[(size_t)jn * nin + i] = best;
        }
        prev_d = bi < 0 ? INFINITY : best;
        prev_i = bi;
    }
}

// knn_density_kernel with a z: the float mean of the neighbours (one chain of additions per coordinate, in neighbour
// order), r = the largest correctly rounded distance from it; the volume and the division as in 2-D
__global__ __launch_bounds__(256) void knn_density3_kernel(const float *__restrict__ pts, int n, int knn,
                                                           const int *__restrict__ ids, float *__restrict__ dens)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n)
        return;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    int real = 0;
    for (int j = 0; j < knn; ++j) {
        const int id = ids[(size_t)j * n + i];
        if (id >= 0) {
            const float *q = pts + 3 * (size_t)id;
            sx = f_add(sx, q[0]);
            sy = f_add(sy, q[1]);
            sz = f_add(sz, q[2]);
            ++real;
        }
    }
    const float mx = __fdiv_rn(sx, (float)real), my = __fdiv_rn(sy, (float)real), mz = __fdiv_rn(sz, (float)real);
    float rmax = 0.0f;
    for (int j = 0; j < knn; ++j) {
        const int id = ids[(size_t)j * n + i];
        if (id >= 0) {
            const float *q = pts + 3 * (size_t)id;
            rmax = fmaxf(rmax, sqrtf(dist2_3(q[0], q[1], q[2], mx, my, mz)));
        }
    }
    const double r = (double)rmax;
    const float volume = (float)((4. / 3.) * 3.14159265358979323846 * (r * r * r));
    dens[i] = __fdiv_rn((float)real, volume);
}

// pcl.remove_outlier: count the points within the radius (itself included); keep iff count > min_points
__global__ __launch_bounds__(256) void radius_count3_kernel(const float *__restrict__ pts, int n, float r2, int min_points,
                                                            int *__restrict__ keep)
{
    __shared__ float s_p[3 * P3_TILE];
    const int i = blockIdx.x * 256 + threadIdx.x;
    float px = 0, py = 0, pz = 0;
    if (i < n) {
        px = pts[3 * (size_t)i];
        py = pts[3 * (size_t)i + 1];
        pz = pts[3 * (size_t)i + 2];
    }
    int cnt = 0;
    for (int tb = 0; tb < n; tb += P3_TILE) {
        const int tn = min(P3_TILE, n - tb);
        __syncthreads();
        p3_stage(s_p, pts, tb, tn);
        __syncthreads();
        for (int j = 0; j < tn; ++j)
            cnt += dist2_3(px, py, pz, s_p[3 * j], s_p[3 * j + 1], s_p[3 * j + 2]) <= r2;
    }
    if (i < n)
        keep[i] = cnt > min_points;
}

// ---------------------------------------------------------------------------------------------
// pcl.downsample on N x 3: the chain of sfe_downsample.hip on an 8-way tree (one cloud per call)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void ds3_bbox_kernel(const float *__restrict__ pts, int n, float max_size,
                                                        Ds3Header *__restrict__ hdr)
{
    __shared__ float s_mn[3][16], s_mx[3][16];
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
        while (!((double)r * 2.0 <= (double)max_size) && L < DS3_MAX_LEVELS) {
            r *= 0.5f;
            ++L;
        }
        hdr->levels = L;
        hdr->n_seg = 0;
    }
}

__global__ __launch_bounds__(256) void ds3_key_kernel(const float *__restrict__ pts, int n, const Ds3Header *__restrict__ hdr,
                                                      unsigned long long *__restrict__ keys)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n)
        return;
    const float px = pts[3 * (size_t)i], py = pts[3 * (size_t)i + 1], pz = pts[3 * (size_t)i + 2];
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
    keys[i] = key;
}

// rank of (key_i, i) among all points = position in the stable sort; scatter index and key there
__global__ __launch_bounds__(256) void ds3_rank_kernel(const unsigned long long *__restrict__ keys, int n,
                                                       int *__restrict__ sorted_idx,
                                                       unsigned long long *__restrict__ sorted_key)
{
    __shared__ unsigned long long s_k[P3_TILE];
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
        sorted_idx[rank] = i;
        sorted_key[rank] = ki;
    }
}

// one workgroup: the first position of every run of equal keys, listed in order, + a sentinel
__global__ __launch_bounds__(1024) void ds3_segment_kernel(const unsigned long long *__restrict__ sorted_key, int n,
                                                           int *__restrict__ seg_start /* [n + 1] */,
                                                           Ds3Header *__restrict__ hdr)
{
    __shared__ int s_part[1024];
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
        hdr->n_seg = s_part[1023];
        seg_start[s_part[1023]] = n; // sentinel (n_seg <= n)
    }
}

// one thread per leaf: float centroid in input order, the first point at the minimum distance from it
__global__ __launch_bounds__(256) void ds3_medoid_kernel(const float *__restrict__ pts, const int *__restrict__ sorted_idx,
                                                         const int *__restrict__ seg_start,
                                                         const Ds3Header *__restrict__ hdr, float *__restrict__ out,
                                                         int *__restrict__ out_idx)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= hdr->n_seg)
        return;
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
        const float d = sqrtf(dist2_3(q[0], q[1], q[2], sx, sy, sz));
        if (d < best) {
            best = d;
            bi = id;
        }
    }
    const float *q = pts + 3 * (size_t)bi;
    out[3 * (size_t)s] = q[0];
    out[3 * (size_t)s + 1] = q[1];
    out[3 * (size_t)s + 2] = q[2];
    out_idx[s] = bi;
}

// the largest cloud whose float offsets (3 n) and [knn x n] tables stay inside the kernels' int arithmetic
#define P3_MAX_POINTS (1 << 28)

extern "C" {

int sfe_match3(sfe_ctx *ctx, const float *ref, int n_ref, const float *in, int n_in, float max_dist, int32_t *ids, float *d2)
{
    return sfe_match_knn3(ctx, ref, n_ref, in, n_in, 1, max_dist, ids, d2);
}

int sfe_match_knn3(sfe_ctx *ctx, const float *ref, int n_ref, const float *in, int n_in, int knn, float max_dist,
                   int32_t *ids, float *d2)
{
    if (int rc = sfe_use(ctx))
        return rc;
    SFE_ARG(ctx, n_ref >= 0 && n_in >= 0 && knn >= 1 && (n_in == 0 || (in && ids && d2)) && (n_ref == 0 || ref));
    SFE_ARG(ctx, n_ref <= P3_MAX_POINTS && n_in <= P3_MAX_POINTS);
    if (n_in == 0)
        return 0;
    const size_t b_ref = sizeof(float) * 3 * (size_t)n_ref, b_in = sizeof(float) * 3 * (size_t)n_in;
    const size_t n_res = (size_t)n_in * (size_t)knn;
    float *d_ref = (float *)sfe_scratch(ctx, 0, std::max(b_ref, sizeof(float) * 3));
    float *d_in = (float *)sfe_scratch(ctx, 1, b_in);
    int *d_ids = (int *)sfe_scratch(ctx, 2, sizeof(int) * n_res);
    float *d_d2 = (float *)sfe_scratch(ctx, 3, sizeof(float) * n_res);
    if (!d_ref || !d_in || !d_ids || !d_d2)
        return SFE_ERR_HIP;
    if (n_ref)
        SFE_HIP(ctx, hipMemcpyAsync(d_ref, ref, b_ref, hipMemcpyHostToDevice, ctx->stream));
    SFE_HIP(ctx, hipMemcpyAsync(d_in, in, b_in, hipMemcpyHostToDevice, ctx->stream));
    const float r2 = max_dist * max_dist; // as sfe_match forms it
    if (knn == 1)
        hipLaunchKernelGGL(match3_kernel, dim3((n_in + 255) / 256), dim3(256), 0, ctx->stream, (const float *)d_ref, n_ref,
                           (const float *)d_in, n_in, r2, d_ids, d_d2);
    else
        hipLaunchKernelGGL(match_knn3_kernel, dim3((n_in + 255) / 256), dim3(256), 0, ctx->stream, (const float *)d_ref, n_ref,
                           (const float *)d_in, n_in, knn, r2, d_ids, d_d2);
    SFE_LAUNCH_CHECK(ctx);
    SFE_HIP(ctx, hipMemcpyAsync(ids, d_ids, sizeof(int) * n_res, hipMemcpyDeviceToHost, ctx->stream));
    SFE_HIP(ctx, hipMemcpyAsync(d2, d_d2, sizeof(float) * n_res, hipMemcpyDeviceToHost, ctx->stream));
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int sfe_knn_density3(sfe_ctx *ctx, const float *pts, int n, int knn, float *dens_out)
{
    if (int rc = sfe_use(ctx))
        return rc;
    SFE_ARG(ctx, n >= 0 && n <= P3_MAX_POINTS && knn >= 1 && (n == 0 || (pts && dens_out)));
    if (n == 0)
        return 0;
    if (knn > n) // libnabo: "Requesting more points than available in cloud"
        return sfe_set_err(ctx, SFE_ERR_ARG, "knn density: %d neighbours requested from a cloud of %d points", knn, n);
    float *d_pts = (float *)sfe_scratch(ctx, 0, sizeof(float) * 3 * (size_t)n);
    int *d_ids = (int *)sfe_scratch(ctx, 2, sizeof(int) * (size_t)n * knn);
    float *d_d2 = (float *)sfe_scratch(ctx, 3, sizeof(float) * (size_t)n * knn);
    float *d_dens = (float *)sfe_scratch(ctx, 1, sizeof(float) * (size_t)n);
    if (!d_pts || !d_ids || !d_d2 || !d_dens)
        return SFE_ERR_HIP;
    SFE_HIP(ctx, hipMemcpyAsync(d_pts, pts, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(match_knn3_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, (const float *)d_pts, n,
                       (const float *)d_pts, n, knn, INFINITY, d_ids, d_d2);
    hipLaunchKernelGGL(knn_density3_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, (const float *)d_pts, n, knn,
                       (const int *)d_ids, d_dens);
    SFE_LAUNCH_CHECK(ctx);
    SFE_HIP(ctx, hipMemcpyAsync(dens_out, d_dens, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int sfe_remove_outlier3(sfe_ctx *ctx, const float *pts, int n, double radius, int min_points, float *out, int *n_out)
{
    if (int rc = sfe_use(ctx))
        return rc;
    SFE_ARG(ctx, n >= 0 && n <= P3_MAX_POINTS && n_out && (n == 0 || (pts && out)));
    *n_out = 0;
    if (n == 0)
        return 0;
    float *d_pts = (float *)sfe_scratch(ctx, 0, sizeof(float) * 3 * (size_t)n);
    int *d_keep = (int *)sfe_scratch(ctx, 2, sizeof(int) * (size_t)n);
    if (!d_pts || !d_keep)
        return SFE_ERR_HIP;
    SFE_HIP(ctx, hipMemcpyAsync(d_pts, pts, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(radius_count3_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, (const float *)d_pts, n,
                       (float)(radius * radius), min_points, d_keep);
    SFE_LAUNCH_CHECK(ctx);
    std::vector<int> keep((size_t)n);
    SFE_HIP(ctx, hipMemcpyAsync(keep.data(), d_keep, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    int m = 0;
    for (int i = 0; i < n; ++i) // order-preserving gather of the kept rows (the decision is the GPU's)
        if (keep[i]) {
            out[3 * (size_t)m] = pts[3 * (size_t)i];
            out[3 * (size_t)m + 1] = pts[3 * (size_t)i + 1];
            out[3 * (size_t)m + 2] = pts[3 * (size_t)i + 2];
            ++m;
        }
    *n_out = m;
    return 0;
}

int sfe_downsample3(sfe_ctx *ctx, const float *pts, int n, float resolution, float *out, int32_t *out_idx, int *n_out)
{
    if (int rc = sfe_use(ctx))
        return rc;
    SFE_ARG(ctx, n >= 0 && n <= P3_MAX_POINTS && n_out && (n == 0 || (pts && out && out_idx)));
    *n_out = 0;
    if (n == 0)
        return 0; // pcl.cpp:130-131
    char buf[64];
    snprintf(buf, sizeof buf, "%f", (double)resolution); // pcl.cpp:134: std::to_string(float)
    const float max_size = strtof(buf, nullptr);
    const size_t b_pts = sizeof(float) * 3 * (size_t)n;
    float *d_pts = (float *)sfe_scratch(ctx, 0, b_pts);
    unsigned long long *d_keys = (unsigned long long *)sfe_scratch(ctx, 1, 8 * (size_t)n);
    unsigned long long *d_skeys = (unsigned long long *)sfe_scratch(ctx, 2, 8 * (size_t)n);
    int *d_sidx = (int *)sfe_scratch(ctx, 3, 4 * (size_t)n);
    int *d_seg = (int *)sfe_scratch(ctx, 4, 4 * ((size_t)n + 1));
    float *d_out = (float *)sfe_scratch(ctx, 5, b_pts);
    int *d_oidx = (int *)sfe_scratch(ctx, 6, 4 * (size_t)n);
    Ds3Header *d_hdr = (Ds3Header *)sfe_scratch(ctx, 7, sizeof(Ds3Header));
    if (!d_pts || !d_keys || !d_skeys || !d_sidx || !d_seg || !d_out || !d_oidx || !d_hdr)
        return SFE_ERR_HIP;
    SFE_HIP(ctx, hipMemcpyAsync(d_pts, pts, b_pts, hipMemcpyHostToDevice, ctx->stream));
    const unsigned nb = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(ds3_bbox_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const float *)d_pts, n, max_size, d_hdr);
    hipLaunchKernelGGL(ds3_key_kernel, dim3(nb), dim3(256), 0, ctx->stream, (const float *)d_pts, n, (const Ds3Header *)d_hdr,
                       d_keys);
    hipLaunchKernelGGL(ds3_rank_kernel, dim3(nb), dim3(256), 0, ctx->stream, (const unsigned long long *)d_keys, n, d_sidx,
                       d_skeys);
    hipLaunchKernelGGL(ds3_segment_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const unsigned long long *)d_skeys, n, d_seg,
                       d_hdr);
    hipLaunchKernelGGL(ds3_medoid_kernel, dim3(nb), dim3(256), 0, ctx->stream, (const float *)d_pts, (const int *)d_sidx,
                       (const int *)d_seg, (const Ds3Header *)d_hdr, d_out, d_oidx);
    SFE_LAUNCH_CHECK(ctx);
    Ds3Header h;
    SFE_HIP(ctx, hipMemcpyAsync(&h, d_hdr, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int m = h.n_seg;
    if (m < 0 || m > n)
        return sfe_set_err(ctx, SFE_ERR_HIP, "downsample3: %d leaves for %d points", m, n);
    SFE_HIP(ctx, hipMemcpyAsync(out, d_out, sizeof(float) * 3 * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    SFE_HIP(ctx, hipMemcpyAsync(out_idx, d_oidx, 4 * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_out = m;
    return 0;
}

} // extern "C"
