// The cloud functions of bruce_slam.pcl on N x 3 clouds: match, remove_outlier, knn_density and downsample
// (pcl.cpp:54-74, 76-88, 128-174 are dimension-generic: fromEigen labels a z row when mat.cols() == 3 and every function
// returns topRows(mat_in.cols())).  The reference carries such clouds (Keyframe.points3D, slam_objects.py:101-106).
//
// match, k-NN, density and radius count are the 3-D counterparts of match_kernel / match_knn_kernel / knn_density_kernel /
// radius_count_kernel (sfe_icp.hip), written as kernels of their own: the 2-D kernels and their launchers are untouched.
// The rules are the 2-D rules with one more coordinate (p3_dist2 of sfe_points3.h).  downsample is a
// one-job call of the octree chain of sfe_octree3.hip.
// Points are packed float triples (12-byte stride, a contiguous N x 3 float32 array): no padding is asked of the caller,
// and nothing is read as float4.  The reference cloud / the point tile goes through LDS, 2048 points (24 KiB) at a time;
// all lanes read the same LDS word in the inner loop (a broadcast).  Every kernel is brute force and quadratic in the
// cloud size, like its 2-D counterpart.  The largest cloud is S3_MAX_POINTS: its float offsets (3 n) and [knn x n] tables
// stay inside the kernels' int arithmetic.
#include "sfe_octree3.h"
#include "sfe_points3.h"

#include <algorithm>
#include <vector>

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
    float best;
    int bi;
    p3_nearest(s_ref, ref, nref, px, py, pz, best, bi);
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
                const float d = p3_dist2(px, py, pz, s_ref[3 * j], s_ref[3 * j + 1], s_ref[3 * j + 2]);
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
            rmax = fmaxf(rmax, sqrtf(p3_dist2(q[0], q[1], q[2], mx, my, mz)));
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
            cnt += p3_dist2(px, py, pz, s_p[3 * j], s_p[3 * j + 1], s_p[3 * j + 2]) <= r2;
    }
    if (i < n)
        keep[i] = cnt > min_points;
}

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
    SFE_ARG(ctx, n_ref <= S3_MAX_POINTS && n_in <= S3_MAX_POINTS);
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
    SFE_ARG(ctx, n >= 0 && n <= S3_MAX_POINTS && knn >= 1 && (n == 0 || (pts && dens_out)));
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
    SFE_ARG(ctx, n >= 0 && n <= S3_MAX_POINTS && n_out && (n == 0 || (pts && out)));
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
    SFE_ARG(ctx, n >= 0 && n <= S3_MAX_POINTS && n_out && (n == 0 || (pts && out && out_idx)));
    *n_out = 0;
    if (n == 0)
        return 0; // pcl.cpp:130-131
    // one job of the octree chain (sfe_octree3.hip): the cloud is its own concatenation
    const float max_size = sfe_s3_max_size(resolution);
    const size_t b_pts = sizeof(float) * 3 * (size_t)n;
    float *d_pts = (float *)sfe_scratch(ctx, 0, b_pts);
    unsigned long long *d_keys = (unsigned long long *)sfe_scratch(ctx, 1, 8 * (size_t)n);
    unsigned long long *d_skeys = (unsigned long long *)sfe_scratch(ctx, 2, 8 * (size_t)n);
    int *d_sidx = (int *)sfe_scratch(ctx, 3, 4 * (size_t)n);
    int *d_seg = (int *)sfe_scratch(ctx, 4, 4 * ((size_t)n + 1));
    float *d_out = (float *)sfe_scratch(ctx, 5, b_pts);
    int *d_oidx = (int *)sfe_scratch(ctx, 6, 4 * (size_t)n);
    S3Header *d_hdr = (S3Header *)sfe_scratch(ctx, 7, sizeof(S3Header));
    S3Job *d_job = (S3Job *)sfe_scratch(ctx, 8, sizeof(S3Job));
    S3Job *h_job = (S3Job *)sfe_pinned_io(ctx, 2, sizeof(S3Job)); // (pinned and the context's: no copy from dead memory)
    if (!d_pts || !d_keys || !d_skeys || !d_sidx || !d_seg || !d_out || !d_oidx || !d_hdr || !d_job || !h_job)
        return SFE_ERR_HIP;
    *h_job = S3Job{0, n, 0, 0, 0};
    SFE_HIP(ctx, hipMemcpyAsync(d_job, h_job, sizeof(S3Job), hipMemcpyHostToDevice, ctx->stream));
    SFE_HIP(ctx, hipMemcpyAsync(d_pts, pts, b_pts, hipMemcpyHostToDevice, ctx->stream));
    if (int rc = sfe_s3_octree_enqueue(ctx, d_pts, d_job, 1, n, max_size,
                                       S3OctreeBufs{d_keys, d_skeys, d_sidx, d_seg, d_hdr, d_out, d_oidx}))
        return rc;
    S3Header h;
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
