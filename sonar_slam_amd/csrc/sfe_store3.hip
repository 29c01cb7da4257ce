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
//   get_points   n_jobs targets per call, every stage ONE launch with the job in blockIdx.y: transform + gather here, then
//                the octree downsample, the offsets and the placement of sfe_octree3.hip (the kernels pcl.downsample on
//                N x 3 runs, so a job's result is bit for bit pcl.downsample of its concatenation).  The results are placed
//                one behind the other at the pool's fill level; the host synchronises once, for the counts.
//   icp          icp3_job_kernel (sfe_icp3.hip) on the pool, its job table built from the slot table: no point is copied.
//   overlap      one lane per moved source point, the target tiled through LDS (2048 points), integer counts.
//
//   keyed clouds (slam.py:229-292 with return_keys, slam_ros.py:317-359; the candidate selection of the loop-closure search,
//   slam.py:873-902 and :977-997): an int32 key and a selection byte per pool point in two pools parallel to the point pool,
//   indexed by the same offsets and allocated at the first keyed call; a `keyed` and a `selected` flag per slot on the host.
//   get_points_keys   the get_points stages with a tag per point: s3_gather_kernel<true> writes the cloud's key next to the
//                     moved point, s3_medoid_kernel<true> also leaves the medoid's index in the concatenation and
//                     s3_pick_keys_kernel picks the leaf's tag through it (the descriptor overload of pcl.downsample);
//                     s3_place_keys_kernel puts the tags into the key pool at the points' offsets.  The <false>
//                     instantiations are the kernels get_points always ran.
//   fov_select        s3_fov_kernel: one lane per point, the job's frames looped; ballot + one atomic per wave for the two
//                     counters, integer atomics into the job's histogram.
//   compact_selected  s3_compact_kernel: one workgroup per cloud, chunks of 1024 with a running base, order kept; the sizes
//                     and the results go through the offsets and place steps, as get_points' do.
//   match_keys        s3_match_keys_kernel: the nearest target of every moved source point (p3_nearest, the scan of
//                     match3_kernel) and the histogram of its key.
//   Every keyed call takes n_jobs jobs and runs one launch per stage for all of them; every call that creates slots asks
//   Store3Slots::fits for an upper bound first.  All counts are integers: no result depends on the order of the atomics; the
//   histogram and counter scratch is zeroed on the stream per call.
//
// The transform rule is numpy's for float32 arrays (sgemm, then the broadcast addition), per output coordinate i
//     fl( fma(p2, Hi2, fma(p1, Hi1, fl(p0 * Hi0))) + Hi3 )
// -- the 3-term form of SFE_STORE_F32_POINTS in sfe_store.hip -- written with explicit intrinsics.
#include "sfe_octree3.h"
#include "sfe_points3.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

struct sfe_cloud_store3 {
    sfe_ctx *ctx = nullptr;
    float *d_pool = nullptr;   // [capacity][3]
    int32_t *d_key = nullptr;  // [capacity]: a key per pool point, at the point's offset (allocated at the first keyed call)
    uint8_t *d_sel = nullptr;  // [capacity]: a selection byte per pool point (allocated with d_key)
    Store3Slots slots;
};

struct S3Pair { // one overlap / match_keys job
    long long src, tgt; // first points in the pool
    int ns, nt;
    float H[12];
};

struct S3FovFrame { // one source frame of the field-of-view gate
    float H[12];    // rows 0..2 of the inverse pose
    double range_bound, bearing_bound;
};

struct S3FovJob { // one keyed cloud against frames [f0, f1)
    long long off;
    int n, f0, f1;
    int pad;
};

// row i of the transform on a point: numpy's float32 `p.dot(R.T) + t`.  Not affine3 of sfe_icp3.hip: numpy's sgemm fuses
// the second and third product into the sum, the ICP kernel's rule rounds every product.
__device__ __forceinline__ float s3_move(const float *row, float p0, float p1, float p2)
{
    return f_add(__fmaf_rn(p2, row[2], __fmaf_rn(p1, row[1], f_mul(p0, row[0]))), row[3]);
}

// ---------------------------------------------------------------------------------------------------------------------
// get_points
// ---------------------------------------------------------------------------------------------------------------------
// transform + gather: point i of job blockIdx.y's concatenation <- its cloud's point, moved; TAG: and its cloud's key
template <bool TAG>
__global__ __launch_bounds__(256) void s3_gather_kernel(const float *__restrict__ pool, const S3Job *__restrict__ jobs,
                                                        const S3Seg *__restrict__ segs, float *__restrict__ cat,
                                                        const int32_t *__restrict__ seg_key, int32_t *__restrict__ cat_key)
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
    if (TAG)
        cat_key[J.cat + i] = seg_key[J.seg0 + k];
}

// the descriptor overload of the downsample: leaf s of job blockIdx.y carries the key of its medoid, picked through the
// medoid's index in the concatenation
__global__ __launch_bounds__(256) void s3_pick_keys_kernel(const int32_t *__restrict__ cat_key, const S3Job *__restrict__ jobs,
                                                           const int *__restrict__ idx_all, const S3Header *__restrict__ hdrs,
                                                           int32_t *__restrict__ out_key)
{
    const S3Job J = jobs[blockIdx.y];
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= hdrs[blockIdx.y].n_seg) // (n_seg <= tot)
        return;
    const int id = idx_all[J.cat + s]; // (in [0, tot): a member of the leaf)
    out_key[J.cat + s] = cat_key[J.cat + id];
}

// the jobs' keys into the key pool, at the offsets s3_place_kernel (sfe_octree3.hip) puts their points
__global__ __launch_bounds__(256) void s3_place_keys_kernel(const int32_t *__restrict__ from, const S3Job *__restrict__ jobs,
                                                            const int *__restrict__ out_cnt,
                                                            const long long *__restrict__ out_off, long long top,
                                                            int32_t *__restrict__ key_pool)
{
    const S3Job J = jobs[blockIdx.y];
    const int n = out_cnt[blockIdx.y]; // (<= tot)
    const int32_t *__restrict__ src = from + J.cat;
    int32_t *__restrict__ dst = key_pool + (top + out_off[blockIdx.y]);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += 256 * gridDim.x)
        dst[i] = src[i];
}

// ---------------------------------------------------------------------------------------------------------------------
// overlap: moved source points with a target point within the radius (the rules of match3_kernel)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void s3_overlap_kernel(const float *__restrict__ pool, const S3Pair *__restrict__ pairs,
                                                         float r2, int *__restrict__ counts)
{
    __shared__ float s_t[3 * P3_TILE];
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
    for (int tb = 0; tb < J.nt; tb += P3_TILE) {
        const int tn = min(P3_TILE, J.nt - tb);
        __syncthreads();
        p3_stage(s_t, tgt, tb, tn);
        __syncthreads();
        for (int j = 0; j < tn; ++j) // every lane reads the same LDS words: a broadcast
            hit |= p3_dist2(px, py, pz, s_t[3 * j], s_t[3 * j + 1], s_t[3 * j + 2]) <= r2; // NaN: never
    }
    hit = hit && i < J.ns;
    const unsigned long long b = __ballot(hit);
    if ((threadIdx.x & 63) == 0 && b)
        atomicAdd(&counts[blockIdx.y], (int)__popcll(b));
}

// ---------------------------------------------------------------------------------------------------------------------
// keyed clouds: the field-of-view gate, the compaction of a selection, the matched targets' keys
// ---------------------------------------------------------------------------------------------------------------------
// The gate of the loop-closure search (slam.py:875-899) with one more coordinate in the transform and the range: for every
// point p of job blockIdx.y's cloud and every frame f of the job
//     q = p moved by the frame's inverse pose (s3_move)
//     range = sqrtf(fl(fl(fl(qx qx) + fl(qy qy)) + fl(qz qz)))         np.linalg.norm(local, axis=1) on float32 N x 3
//     f sees p  iff  (double)range < range_bound  and  |atan2(qy, qx)| < bearing_bound        the horizontal bearing
// and p is selected iff some frame sees it.  sqrtf, not __fsqrt_rn: the correctly rounded sequence (store_fov_kernel of
// sfe_store.hip says why).  numpy's float32 arctan2 is libm's atan2f, whose last bit is not reproduced here: atan2 runs in
// double and decides only outside 1e-6 a + 1e-30 of the bound; a point that no frame selects for certain and some frame
// leaves undecided counts as ambiguous and stays unselected (the host then takes the numpy path for this cloud).
// One lane per point; the counters by ballot + one atomic per wave, the histogram by integer atomics: no order dependence.
__global__ __launch_bounds__(256) void s3_fov_kernel(const float *__restrict__ pool, const int32_t *__restrict__ key_pool,
                                                     const S3FovJob *__restrict__ jobs, const S3FovFrame *__restrict__ frames,
                                                     int n_keys, uint8_t *__restrict__ sel_pool, int32_t *__restrict__ hist_,
                                                     int32_t *__restrict__ counters_ /* [j][0] selected, [j][1] ambiguous */)
{
    const int j = blockIdx.y;
    const S3FovJob jb = jobs[j];
    if (blockIdx.x * 256 >= jb.n) // (uniform: the whole workgroup -- a cloud smaller than the largest of the call)
        return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool yes = false, maybe = false;
    if (i < jb.n) {
        const float *p = pool + 3 * (size_t)(jb.off + i);
        const float p0 = p[0], p1 = p[1], p2 = p[2];
        for (int f = jb.f0; f < jb.f1; ++f) {
            const S3FovFrame *fr = frames + f; // (uniform: scalar loads)
            const float qx = s3_move(fr->H, p0, p1, p2);
            const float qy = s3_move(fr->H + 4, p0, p1, p2);
            const float qz = s3_move(fr->H + 8, p0, p1, p2);
            const float range = sqrtf(f_add(f_add(f_mul(qx, qx), f_mul(qy, qy)), f_mul(qz, qz)));
            if (!((double)range < fr->range_bound)) // (NaN: never)
                continue;
            const double a = fabs(atan2((double)qy, (double)qx));
            const double margin = 1e-6 * a + 1e-30;
            if (a < fr->bearing_bound - margin)
                yes = true;
            else if (!(a > fr->bearing_bound + margin))
                maybe = true;
        }
        sel_pool[jb.off + i] = yes ? 1 : 0;
        if (yes) {
            const int k = key_pool[jb.off + i];
            if (k >= 0 && k < n_keys)
                atomicAdd(&hist_[(size_t)j * n_keys + k], 1);
        }
    }
    const unsigned long long by = __ballot(yes), bm = __ballot(maybe && !yes);
    if ((threadIdx.x & 63) == 0) {
        if (by)
            atomicAdd(&counters_[2 * (size_t)j], (int)__popcll(by));
        if (bm)
            atomicAdd(&counters_[2 * (size_t)j + 1], (int)__popcll(bm));
    }
}

// points[sel], keys[sel] of job blockIdx.x's cloud (the pool points at src[j], jobs[j].tot of them), order kept: one workgroup
// per cloud, chunks of 1024 with a running base.  The survivors go to the job's place in the scratch arrays (jobs[j].cat), their
// number to hdrs[j].n_seg, from where the offsets and place kernels of get_points take them.
__global__ __launch_bounds__(1024) void s3_compact_kernel(const float *__restrict__ pool, const int32_t *__restrict__ key_pool,
                                                          const uint8_t *__restrict__ sel_pool, const S3Job *__restrict__ jobs,
                                                          const long long *__restrict__ src, float *__restrict__ out_all,
                                                          int32_t *__restrict__ out_key_all, S3Header *__restrict__ hdrs)
{
    __shared__ int s_wave[16];
    __shared__ int s_base;
    const S3Job J = jobs[blockIdx.x];
    const long long off = src[blockIdx.x];
    const int n = J.tot;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0)
        s_base = 0;
    __syncthreads();
    for (int b = 0; b < n; b += 1024) { // (uniform trip count)
        const int i = b + tid;
        const bool on = i < n && sel_pool[off + i] != 0;
        const unsigned long long m = __ballot(on);
        if (lane == 0)
            s_wave[wave] = (int)__popcll(m);
        __syncthreads();
        int pre = s_base;
        for (int w = 0; w < wave; ++w)
            pre += s_wave[w];
        if (on) {
            const int pos = pre + (int)__popcll(m & ((1ull << lane) - 1ull)); // (< n: it counts selected points before i)
            const float *p = pool + 3 * (size_t)(off + i);
            float *o = out_all + 3 * (size_t)(J.cat + pos);
            o[0] = p[0];
            o[1] = p[1];
            o[2] = p[2];
            out_key_all[J.cat + pos] = key_pool[off + i];
        }
        __syncthreads();
        if (tid == 0) {
            int t = 0;
            for (int w = 0; w < 16; ++w)
                t += s_wave[w];
            s_base += t;
        }
        __syncthreads();
    }
    if (tid == 0)
        hdrs[blockIdx.x].n_seg = s_base;
}

// get_overlap(..., return_indices=True) and the keys of the matched targets (slam.py:977-985): every moved source point gets
// its sfe_match3 neighbour -- p3_nearest: the nearest target by p3_dist2, the lowest index among equal distances -- kept iff
// d2 <= r2; NaN and infinite distances never win.
// hist[key of the neighbour] += 1; the number of matches is what s3_overlap_kernel counts.
__global__ __launch_bounds__(256) void s3_match_keys_kernel(const float *__restrict__ pool, const int32_t *__restrict__ key_pool,
                                                            const S3Pair *__restrict__ pairs, float r2, int n_keys,
                                                            int32_t *__restrict__ hist_, int32_t *__restrict__ overlap_)
{
    __shared__ float s_t[3 * P3_TILE];
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
    float best;
    int bi;
    p3_nearest(s_t, pool + 3 * (size_t)J.tgt, J.nt, px, py, pz, best, bi);
    const bool hit = i < J.ns && bi >= 0 && best <= r2;
    if (hit) {
        const int k = key_pool[J.tgt + bi];
        if (k >= 0 && k < n_keys)
            atomicAdd(&hist_[(size_t)blockIdx.y * n_keys + k], 1);
    }
    const unsigned long long m = __ballot(hit);
    if ((threadIdx.x & 63) == 0 && m)
        atomicAdd(&overlap_[blockIdx.y], (int)__popcll(m));
}

// ---------------------------------------------------------------------------------------------------------------------
static int s3_check(sfe_ctx *ctx, sfe_cloud_store3 *s)
{
    if (int rc = sfe_use(ctx))
        return rc;
    SFE_ARG(ctx, s && s->ctx == ctx);
    return 0;
}

// The key pool (an int32 per pool point) and the selection pool (a byte per pool point), indexed by the point pool's offsets.
// Allocated at the first keyed call, both or neither: a store that never uses keys costs what it did without them.
static int s3_key_pools(sfe_cloud_store3 *s)
{
    if (s->d_key)
        return 0;
    const size_t n = (size_t)s->slots.capacity;
    int32_t *k = nullptr;
    uint8_t *b = nullptr;
    if (hipMalloc((void **)&k, sizeof(int32_t) * n) != hipSuccess || hipMalloc((void **)&b, n) != hipSuccess) {
        (void)hipGetLastError();
        if (k)
            (void)hipFree(k);
        return sfe_set_err(s->ctx, SFE_ERR_HIP, "3-D cloud store: allocating the key and selection pools (%lld points) failed",
                           (long long)s->slots.capacity);
    }
    s->d_key = k;
    s->d_sel = b;
    return 0;
}

static int s3_keyed_cloud(sfe_cloud_store3 *s, int32_t handle, const char *what)
{
    if (!s->slots.valid(handle))
        return sfe_set_err(s->ctx, SFE_ERR_ARG, "3-D %s names cloud %d, the store holds %d", what, handle, s->slots.n_slots);
    if (!s->slots.is_keyed(handle))
        return sfe_set_err(s->ctx, SFE_ERR_ARG, "3-D %s: cloud %d has no keys (a cloud from put or get_points)", what, handle);
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
    if (s->d_key)
        (void)hipFree(s->d_key);
    if (s->d_sel)
        (void)hipFree(s->d_sel);
    delete s;
}

int sfe_cloud_store3_count(sfe_cloud_store3 *s) { return s ? s->slots.n_slots : 0; }

// put and put_keys (keys != nullptr)
static int s3_put(sfe_ctx *ctx, sfe_cloud_store3 *s, int64_t stamp, const float *pts, const int32_t *keys, int n,
                  int32_t *handle_out)
{
    Store3Slots &t = s->slots;
    const S3Bound need = s3_bound_put(n);
    if (!t.fits(need.points, need.slots))
        return sfe_set_err(ctx, SFE_ERR_CAP, "3-D cloud store: a cloud of %d points does not fit (%lld of %lld points and %d of "
                                             "%d slots in use)", n, (long long)t.top, (long long)t.capacity, t.n_slots, t.max_clouds);
    if (keys)
        if (int rc = s3_key_pools(s))
            return rc;
    if (n) {
        // through the event-guarded pinned staging: the caller's arrays may go away when the call returns
        const size_t b_pts = sizeof(float) * 3 * (size_t)n, b_key = keys ? sizeof(int32_t) * (size_t)n : 0;
        char *h = (char *)sfe_pinned_begin(ctx, b_pts + b_key);
        if (!h)
            return SFE_ERR_HIP;
        memcpy(h, pts, b_pts);
        SFE_HIP(ctx, hipMemcpyAsync(s->d_pool + 3 * (size_t)t.top, h, b_pts, hipMemcpyHostToDevice, ctx->stream));
        if (keys) {
            memcpy(h + b_pts, keys, b_key);
            SFE_HIP(ctx, hipMemcpyAsync(s->d_key + (size_t)t.top, h + b_pts, b_key, hipMemcpyHostToDevice, ctx->stream));
        }
        if (int rc = sfe_pinned_end(ctx, ctx->stream))
            return rc;
    }
    *handle_out = t.push(stamp, n, keys != nullptr);
    return 0;
}

int sfe_cloud_store3_put(sfe_ctx *ctx, sfe_cloud_store3 *s, int64_t stamp, const float *pts, int n, int32_t *handle_out)
{
    if (int rc = s3_check(ctx, s))
        return rc;
    SFE_ARG(ctx, n >= 0 && n <= S3_MAX_POINTS && (n == 0 || pts) && handle_out);
    return s3_put(ctx, s, stamp, pts, nullptr, n, handle_out);
}

int sfe_cloud_store3_put_keys(sfe_ctx *ctx, sfe_cloud_store3 *s, int64_t stamp, const float *pts, const int32_t *keys, int n,
                              int32_t *handle_out)
{
    static const int32_t no_keys[1] = {0};
    if (int rc = s3_check(ctx, s))
        return rc;
    SFE_ARG(ctx, n >= 0 && n <= S3_MAX_POINTS && (n == 0 || (pts && keys)) && handle_out);
    for (int i = 0; i < n; ++i)
        if (keys[i] < 0)
            return sfe_set_err(ctx, SFE_ERR_ARG, "3-D put_keys: key %d of point %d is negative", keys[i], i);
    return s3_put(ctx, s, stamp, pts, n ? keys : no_keys, n, handle_out);
}

int sfe_cloud_store3_keyed(sfe_cloud_store3 *s, int32_t handle)
{
    if (!s || !s->slots.valid(handle))
        return SFE_ERR_ARG;
    return s->slots.is_keyed(handle) ? 1 : 0;
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

// get_points (keys == nullptr) and get_points_keys: job j lists the entries [job_off[j], job_off[j + 1])
static int s3_get_points(sfe_ctx *ctx, sfe_cloud_store3 *s, const int32_t *handles, const float *H12, const int32_t *keys,
                         const int64_t *job_off, int n_jobs, float resolution, const int64_t *stamps, int32_t *handles_out,
                         const char *what)
{
    Store3Slots &t = s->slots;
    S3JobTable tab;
    int bad_job = 0;
    int64_t bad_entry = 0;
    switch (s3_build_jobs(t, handles, H12, keys, job_off, n_jobs, tab, &bad_job, &bad_entry)) {
    case S3_JOBS_OK:
        break;
    case S3_JOBS_BAD_HANDLE:
        return sfe_set_err(ctx, SFE_ERR_ARG, "3-D %s: job %d names cloud %d, the store holds %d", what, bad_job,
                           handles[bad_entry], t.n_slots);
    case S3_JOBS_TOO_MANY_POINTS:
        return sfe_set_err(ctx, SFE_ERR_ARG, "3-D %s: job %d concatenates more than %d points", what, bad_job, S3_MAX_POINTS);
    case S3_JOBS_BAD_KEY:
        return sfe_set_err(ctx, SFE_ERR_ARG, "3-D %s: job %d tags cloud %d with the negative key %d", what, bad_job,
                           handles[bad_entry], keys[bad_entry]);
    default:
        return sfe_set_err(ctx, SFE_ERR_ARG, "3-D %s: the entries of job %d do not follow those of the job before it", what,
                           bad_job);
    }
    const std::vector<S3Job> &jobs = tab.jobs;
    const std::vector<S3Seg> &segs = tab.segs;
    const int64_t total = tab.total;
    const int max_tot = tab.max_tot;
    // the call's upper bound: no downsample leaves more points than it was given
    const S3Bound need = s3_bound_get_points(tab);
    if (!t.fits(need.points, need.slots))
        return sfe_set_err(ctx, SFE_ERR_CAP, "3-D %s: %d clouds of up to %lld points in all do not fit (%lld of %lld points "
                                             "and %d of %d slots in use)", what, n_jobs, (long long)total, (long long)t.top,
                           (long long)t.capacity, t.n_slots, t.max_clouds);
    if (keys)
        if (int rc = s3_key_pools(s))
            return rc;
    const int raw = !(resolution > 0.0f);
    const float max_size = sfe_s3_max_size(resolution);

    const size_t np = (size_t)std::max<int64_t>(total, 1);
    const size_t b_jobs = sizeof(S3Job) * (size_t)n_jobs, b_segs = sizeof(S3Seg) * segs.size();
    const size_t b_skey = keys ? sizeof(int32_t) * segs.size() : 0, b_tab = b_jobs + b_segs + b_skey;
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
    // with keys: the tag of every point of the concatenations, the medoids' indices and the medoids' tags
    int32_t *d_ckey = nullptr, *d_okey = nullptr;
    int *d_midx = nullptr;
    if (keys) {
        d_ckey = (int32_t *)sfe_scratch(ctx, 9, 4 * np);
        d_okey = (int32_t *)sfe_scratch(ctx, 10, 4 * np);
        d_midx = (int *)sfe_scratch(ctx, 11, 4 * np);
        if (!d_ckey || !d_okey || !d_midx)
            return SFE_ERR_HIP;
    }
    memcpy(h_tab, jobs.data(), b_jobs);
    if (b_segs)
        memcpy(h_tab + b_jobs, segs.data(), b_segs);
    if (b_skey)
        memcpy(h_tab + b_jobs + b_segs, tab.seg_key.data(), b_skey);
    SFE_HIP(ctx, hipMemcpyAsync(d_tab, h_tab, b_tab, hipMemcpyHostToDevice, ctx->stream));
    const S3Job *d_jobs = (const S3Job *)d_tab;
    const S3Seg *d_segs = (const S3Seg *)(d_tab + b_jobs);
    const int32_t *d_segkey = (const int32_t *)(d_tab + b_jobs + b_segs);
    long long *d_off = (long long *)d_place;
    int32_t *d_cnt = (int32_t *)(d_place + sizeof(long long) * (size_t)n_jobs);
    const unsigned nb = (unsigned)std::max((max_tot + 255) / 256, 1);
    const dim3 per_point(nb, (unsigned)n_jobs);
    if (keys)
        hipLaunchKernelGGL(s3_gather_kernel<true>, per_point, dim3(256), 0, ctx->stream, (const float *)s->d_pool, d_jobs, d_segs,
                           d_cat, d_segkey, d_ckey);
    else
        hipLaunchKernelGGL(s3_gather_kernel<false>, per_point, dim3(256), 0, ctx->stream, (const float *)s->d_pool, d_jobs, d_segs,
                           d_cat, (const int32_t *)nullptr, (int32_t *)nullptr);
    if (!raw) {
        if (int rc = sfe_s3_octree_enqueue(ctx, d_cat, d_jobs, n_jobs, max_tot, max_size,
                                           S3OctreeBufs{d_keys, d_skeys, d_sidx, d_seg, d_hdr, d_out, d_midx}))
            return rc;
        if (keys)
            hipLaunchKernelGGL(s3_pick_keys_kernel, per_point, dim3(256), 0, ctx->stream, (const int32_t *)d_ckey, d_jobs,
                               (const int *)d_midx, (const S3Header *)d_hdr, d_okey);
    }
    if (int rc = sfe_s3_offsets_enqueue(ctx, d_jobs, d_hdr, n_jobs, raw, d_cnt, d_off))
        return rc;
    // (the results lie within [top, top + total): the sum of the jobs' sizes is at most the bound tested above)
    if (int rc = sfe_s3_place_enqueue(ctx, raw ? d_cat : d_out, d_jobs, n_jobs, max_tot, d_cnt, d_off, (long long)t.top,
                                      s->d_pool))
        return rc;
    if (keys)
        hipLaunchKernelGGL(s3_place_keys_kernel, dim3(std::min(nb, 64u), (unsigned)n_jobs), dim3(256), 0, ctx->stream,
                           (const int32_t *)(raw ? d_ckey : d_okey), d_jobs, (const int *)d_cnt, (const long long *)d_off,
                           (long long)t.top, s->d_key);
    SFE_LAUNCH_CHECK(ctx);
    SFE_HIP(ctx, hipMemcpyAsync(h_cnt, d_cnt, b_cnt, hipMemcpyDeviceToHost, ctx->stream));
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the call's one synchronisation: the sizes
    for (int j = 0; j < n_jobs; ++j)
        if (h_cnt[j] < 0 || h_cnt[j] > jobs[(size_t)j].tot || (jobs[(size_t)j].tot > 0 && h_cnt[j] == 0))
            return sfe_set_err(ctx, SFE_ERR_HIP, "3-D %s: job %d left %d points of %d", what, j, h_cnt[j], jobs[(size_t)j].tot);
    for (int j = 0; j < n_jobs; ++j)
        handles_out[j] = t.push(stamps ? stamps[j] : 0, h_cnt[j], keys != nullptr);
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
    std::vector<int64_t> job_off((size_t)n_jobs + 1);
    for (int j = 0; j <= n_jobs; ++j)
        job_off[(size_t)j] = (int64_t)j * m;
    return s3_get_points(ctx, s, handles, H12, nullptr, job_off.data(), n_jobs, resolution, stamps, handles_out, "get_points");
}

int sfe_cloud_store3_get_points_keys(sfe_ctx *ctx, sfe_cloud_store3 *s, const int32_t *handles, const float *H12,
                                     const int32_t *keys, const int32_t *job_off, int n_jobs, float resolution,
                                     const int64_t *stamps, int32_t *handles_out)
{
    if (int rc = s3_check(ctx, s))
        return rc;
    SFE_ARG(ctx, n_jobs >= 0 && n_jobs <= S3_MAX_JOBS && (n_jobs == 0 || (job_off && handles_out)));
    if (n_jobs == 0)
        return 0;
    SFE_ARG(ctx, job_off[0] == 0 && job_off[n_jobs] >= 0 && (job_off[n_jobs] == 0 || (handles && H12 && keys)));
    static const int32_t none[1] = {0};
    std::vector<int64_t> off64(job_off, job_off + n_jobs + 1);
    return s3_get_points(ctx, s, handles, H12, keys ? keys : none, off64.data(), n_jobs, resolution, stamps, handles_out,
                         "get_points_keys");
}

int sfe_cloud_store3_read_keys(sfe_ctx *ctx, sfe_cloud_store3 *s, int32_t handle, int32_t *out, int cap, int *n_out)
{
    if (int rc = s3_check(ctx, s))
        return rc;
    SFE_ARG(ctx, n_out && cap >= 0 && (cap == 0 || out));
    if (int rc = s3_keyed_cloud(s, handle, "read_keys"))
        return rc;
    const int n = (int)s->slots.cnt[(size_t)handle];
    *n_out = n;
    if (n == 0)
        return 0;
    if (n > cap)
        return sfe_set_err(ctx, SFE_ERR_CAP, "3-D cloud store: cloud %d has %d keys, the buffer holds %d", handle, n, cap);
    SFE_HIP(ctx, hipMemcpyAsync(out, s->d_key + (size_t)s->slots.off[(size_t)handle], sizeof(int32_t) * (size_t)n,
                                hipMemcpyDeviceToHost, ctx->stream));
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int sfe_cloud_store3_fov_select(sfe_ctx *ctx, sfe_cloud_store3 *s, const int32_t *handles, int n_jobs, const float *Hinv12,
                                const double *range_bound, const double *bearing_bound, const int32_t *frame_off, int n_keys,
                                int32_t *key_counts_out, int32_t *n_selected_out, int32_t *n_ambiguous_out)
{
    if (int rc = s3_check(ctx, s))
        return rc;
    SFE_ARG(ctx, n_jobs >= 0 && n_jobs <= S3_MAX_JOBS && n_keys >= 0);
    if (n_jobs == 0)
        return 0;
    SFE_ARG(ctx, handles && frame_off && n_selected_out && n_ambiguous_out && frame_off[0] == 0 && (n_keys == 0 || key_counts_out));
    for (int j = 0; j < n_jobs; ++j) {
        SFE_ARG(ctx, frame_off[j + 1] >= frame_off[j]);
        if (int rc = s3_keyed_cloud(s, handles[j], "fov_select"))
            return rc;
    }
    const int n_frames = frame_off[n_jobs];
    SFE_ARG(ctx, n_frames == 0 || (Hinv12 && range_bound && bearing_bound));
    Store3Slots &t = s->slots;
    const size_t b_fr = sizeof(S3FovFrame) * (size_t)std::max(n_frames, 1), b_job = sizeof(S3FovJob) * (size_t)n_jobs;
    const size_t n_out = 2 * (size_t)n_jobs + (size_t)n_jobs * (size_t)n_keys, b_out = sizeof(int32_t) * n_out;
    char *h_up = (char *)sfe_pinned_io(ctx, 2, b_fr + b_job);
    int32_t *h_out = (int32_t *)sfe_pinned_io(ctx, 3, b_out);
    char *d_up = (char *)sfe_scratch(ctx, 6, b_fr + b_job);
    int32_t *d_out = (int32_t *)sfe_scratch(ctx, 7, b_out);
    if (!h_up || !h_out || !d_up || !d_out)
        return SFE_ERR_HIP;
    S3FovFrame *h_fr = (S3FovFrame *)h_up;
    S3FovJob *h_job = (S3FovJob *)(h_up + b_fr);
    for (int f = 0; f < n_frames; ++f) {
        memcpy(h_fr[f].H, Hinv12 + 12 * (size_t)f, sizeof h_fr[f].H);
        h_fr[f].range_bound = range_bound[f];
        h_fr[f].bearing_bound = bearing_bound[f];
    }
    int n_max = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const size_t h = (size_t)handles[j];
        h_job[j] = S3FovJob{(long long)t.off[h], (int)t.cnt[h], frame_off[j], frame_off[j + 1], 0};
        n_max = std::max(n_max, (int)t.cnt[h]);
    }
    SFE_HIP(ctx, hipMemcpyAsync(d_up, h_up, b_fr + b_job, hipMemcpyHostToDevice, ctx->stream));
    SFE_HIP(ctx, hipMemsetAsync(d_out, 0, b_out, ctx->stream));
    if (n_max > 0) {
        hipLaunchKernelGGL(s3_fov_kernel, dim3((unsigned)((n_max + 255) / 256), (unsigned)n_jobs), dim3(256), 0, ctx->stream,
                           (const float *)s->d_pool, (const int32_t *)s->d_key, (const S3FovJob *)(d_up + b_fr),
                           (const S3FovFrame *)d_up, n_keys, s->d_sel, d_out + 2 * (size_t)n_jobs, d_out);
        SFE_LAUNCH_CHECK(ctx);
    }
    SFE_HIP(ctx, hipMemcpyAsync(h_out, d_out, b_out, hipMemcpyDeviceToHost, ctx->stream));
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int j = 0; j < n_jobs; ++j) {
        t.selected[(size_t)handles[j]] = 1;
        n_selected_out[j] = h_out[2 * j];
        n_ambiguous_out[j] = h_out[2 * j + 1];
    }
    if (n_keys)
        memcpy(key_counts_out, h_out + 2 * (size_t)n_jobs, sizeof(int32_t) * (size_t)n_jobs * (size_t)n_keys);
    return 0;
}

int sfe_cloud_store3_set_selection(sfe_ctx *ctx, sfe_cloud_store3 *s, int32_t handle, const uint8_t *sel, int n)
{
    if (int rc = s3_check(ctx, s))
        return rc;
    SFE_ARG(ctx, n >= 0 && (n == 0 || sel));
    if (int rc = s3_keyed_cloud(s, handle, "set_selection"))
        return rc;
    Store3Slots &t = s->slots;
    SFE_ARG(ctx, (int64_t)n == t.cnt[(size_t)handle]);
    if (n) {
        char *h = (char *)sfe_pinned_begin(ctx, (size_t)n);
        if (!h)
            return SFE_ERR_HIP;
        memcpy(h, sel, (size_t)n);
        SFE_HIP(ctx, hipMemcpyAsync(s->d_sel + (size_t)t.off[(size_t)handle], h, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        if (int rc = sfe_pinned_end(ctx, ctx->stream))
            return rc;
    }
    t.selected[(size_t)handle] = 1;
    return 0;
}

int sfe_cloud_store3_compact_selected(sfe_ctx *ctx, sfe_cloud_store3 *s, const int32_t *handles, int n_jobs,
                                      const int64_t *stamps, int32_t *handles_out)
{
    if (int rc = s3_check(ctx, s))
        return rc;
    SFE_ARG(ctx, n_jobs >= 0 && n_jobs <= S3_MAX_JOBS && (n_jobs == 0 || (handles && handles_out)));
    if (n_jobs == 0)
        return 0;
    Store3Slots &t = s->slots;
    for (int j = 0; j < n_jobs; ++j) {
        if (int rc = s3_keyed_cloud(s, handles[j], "compact_selected"))
            return rc;
        if (!t.has_selection(handles[j]))
            return sfe_set_err(ctx, SFE_ERR_ARG, "3-D compact_selected: cloud %d has no selection (neither fov_select nor "
                                                 "set_selection wrote one)", handles[j]);
    }
    // the call's upper bound: a selection keeps at most every point of its cloud
    const S3Bound need = s3_bound_compact(t, handles, n_jobs);
    if (!t.fits(need.points, need.slots))
        return sfe_set_err(ctx, SFE_ERR_CAP, "3-D compact_selected: %d clouds of up to %lld points in all do not fit (%lld of "
                                             "%lld points and %d of %d slots in use)", n_jobs, (long long)need.points,
                           (long long)t.top, (long long)t.capacity, t.n_slots, t.max_clouds);
    const size_t np = (size_t)std::max<int64_t>(need.points, 1);
    const size_t b_jobs = sizeof(S3Job) * (size_t)n_jobs, b_src = sizeof(long long) * (size_t)n_jobs, b_tab = b_jobs + b_src;
    const size_t b_cnt = sizeof(int32_t) * (size_t)n_jobs;
    char *h_tab = (char *)sfe_pinned_io(ctx, 2, b_tab);
    int32_t *h_cnt = (int32_t *)sfe_pinned_io(ctx, 3, b_cnt);
    float *d_out = (float *)sfe_scratch(ctx, 5, sizeof(float) * 3 * np);
    char *d_tab = (char *)sfe_scratch(ctx, 6, b_tab);
    S3Header *d_hdr = (S3Header *)sfe_scratch(ctx, 7, sizeof(S3Header) * (size_t)n_jobs);
    char *d_place = (char *)sfe_scratch(ctx, 8, (sizeof(long long) + sizeof(int32_t)) * (size_t)n_jobs);
    int32_t *d_okey = (int32_t *)sfe_scratch(ctx, 10, 4 * np);
    if (!h_tab || !h_cnt || !d_out || !d_tab || !d_hdr || !d_place || !d_okey)
        return SFE_ERR_HIP;
    S3Job *h_jobs = (S3Job *)h_tab;
    long long *h_src = (long long *)(h_tab + b_jobs);
    int64_t at = 0;
    int max_n = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const size_t h = (size_t)handles[j];
        h_jobs[j] = S3Job{(long long)at, (int)t.cnt[h], 0, 0, 0};
        h_src[j] = (long long)t.off[h];
        at += t.cnt[h];
        max_n = std::max(max_n, (int)t.cnt[h]);
    }
    SFE_HIP(ctx, hipMemcpyAsync(d_tab, h_tab, b_tab, hipMemcpyHostToDevice, ctx->stream));
    const S3Job *d_jobs = (const S3Job *)d_tab;
    long long *d_off = (long long *)d_place;
    int32_t *d_cnt = (int32_t *)(d_place + sizeof(long long) * (size_t)n_jobs);
    const unsigned nb = (unsigned)std::max((max_n + 255) / 256, 1);
    hipLaunchKernelGGL(s3_compact_kernel, dim3((unsigned)n_jobs), dim3(1024), 0, ctx->stream, (const float *)s->d_pool,
                       (const int32_t *)s->d_key, (const uint8_t *)s->d_sel, d_jobs, (const long long *)(d_tab + b_jobs), d_out,
                       d_okey, d_hdr);
    if (int rc = sfe_s3_offsets_enqueue(ctx, d_jobs, d_hdr, n_jobs, 0, d_cnt, d_off))
        return rc;
    // (the results lie within [top, top + need.points))
    if (int rc = sfe_s3_place_enqueue(ctx, d_out, d_jobs, n_jobs, max_n, d_cnt, d_off, (long long)t.top, s->d_pool))
        return rc;
    hipLaunchKernelGGL(s3_place_keys_kernel, dim3(std::min(nb, 64u), (unsigned)n_jobs), dim3(256), 0, ctx->stream,
                       (const int32_t *)d_okey, d_jobs, (const int *)d_cnt, (const long long *)d_off, (long long)t.top, s->d_key);
    SFE_LAUNCH_CHECK(ctx);
    SFE_HIP(ctx, hipMemcpyAsync(h_cnt, d_cnt, b_cnt, hipMemcpyDeviceToHost, ctx->stream));
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the call's one synchronisation: the sizes
    for (int j = 0; j < n_jobs; ++j)
        if (h_cnt[j] < 0 || h_cnt[j] > h_jobs[j].tot)
            return sfe_set_err(ctx, SFE_ERR_HIP, "3-D compact_selected: job %d left %d points of %d", j, h_cnt[j], h_jobs[j].tot);
    for (int j = 0; j < n_jobs; ++j)
        handles_out[j] = t.push(stamps ? stamps[j] : 0, h_cnt[j], true);
    return 0;
}

int sfe_cloud_store3_match_keys(sfe_ctx *ctx, sfe_cloud_store3 *s, const int32_t *pairs, const float *H12, int n_jobs,
                                float max_dist, int n_keys, int32_t *key_counts_out, int32_t *overlap_out)
{
    if (int rc = s3_check(ctx, s))
        return rc;
    SFE_ARG(ctx, n_jobs >= 0 && n_jobs <= S3_MAX_JOBS && n_keys >= 0);
    if (n_jobs == 0)
        return 0;
    SFE_ARG(ctx, pairs && H12 && overlap_out && (n_keys == 0 || key_counts_out));
    const Store3Slots &t = s->slots;
    for (int j = 0; j < n_jobs; ++j) {
        if (!t.valid(pairs[2 * j]))
            return sfe_set_err(ctx, SFE_ERR_ARG, "3-D match_keys %d names source cloud %d, the store holds %d", j, pairs[2 * j],
                               t.n_slots);
        if (int rc = s3_keyed_cloud(s, pairs[2 * j + 1], "match_keys"))
            return rc;
    }
    const size_t b_in = sizeof(S3Pair) * (size_t)n_jobs;
    const size_t b_out = sizeof(int32_t) * ((size_t)n_jobs + (size_t)n_jobs * (size_t)n_keys);
    S3Pair *h_in = (S3Pair *)sfe_pinned_io(ctx, 2, b_in);
    int32_t *h_out = (int32_t *)sfe_pinned_io(ctx, 3, b_out);
    S3Pair *d_in = (S3Pair *)sfe_scratch(ctx, 6, b_in);
    int32_t *d_out = (int32_t *)sfe_scratch(ctx, 7, b_out);
    if (!h_in || !h_out || !d_in || !d_out)
        return SFE_ERR_HIP;
    int max_ns = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const size_t hs = (size_t)pairs[2 * j], ht = (size_t)pairs[2 * j + 1];
        S3Pair &q = h_in[j];
        q.src = t.off[hs];
        q.tgt = t.off[ht];
        q.ns = (int)t.cnt[hs];
        q.nt = (int)t.cnt[ht];
        memcpy(q.H, H12 + 12 * (size_t)j, sizeof q.H);
        max_ns = std::max(max_ns, q.ns);
    }
    float r2 = max_dist * max_dist; // as sfe_match forms it; the radius test of sfe_cloud_store3_overlap
    if (r2 > FLT_MAX)
        r2 = FLT_MAX;
    SFE_HIP(ctx, hipMemcpyAsync(d_in, h_in, b_in, hipMemcpyHostToDevice, ctx->stream));
    SFE_HIP(ctx, hipMemsetAsync(d_out, 0, b_out, ctx->stream));
    if (max_ns > 0) {
        hipLaunchKernelGGL(s3_match_keys_kernel, dim3((unsigned)((max_ns + 255) / 256), (unsigned)n_jobs), dim3(256), 0, ctx->stream,
                           (const float *)s->d_pool, (const int32_t *)s->d_key, (const S3Pair *)d_in, r2, n_keys, d_out + n_jobs,
                           d_out);
        SFE_LAUNCH_CHECK(ctx);
    }
    SFE_HIP(ctx, hipMemcpyAsync(h_out, d_out, b_out, hipMemcpyDeviceToHost, ctx->stream));
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(overlap_out, h_out, sizeof(int32_t) * (size_t)n_jobs);
    if (n_keys)
        memcpy(key_counts_out, h_out + n_jobs, sizeof(int32_t) * (size_t)n_jobs * (size_t)n_keys);
    return 0;
}

int sfe_icp3_store_compute(sfe_ctx *ctx, const sfe_icp_params *p, sfe_cloud_store3 *s, const int32_t *pairs,
                           const float *guesses16, int n_jobs, float *T_out16, int32_t *status, int32_t *iters)
{
    return sfe_icp3_store_compute_chain_ext(ctx, p, nullptr, nullptr, 0, nullptr, 0, s, pairs, guesses16, n_jobs, T_out16, status,
                                            iters);
}

// the chain's filters write context scratch only: the store's slots, pool and count stay as they are
int sfe_icp3_store_compute_chain_ext(sfe_ctx *ctx, const sfe_icp_params *p, const sfe_icp_outliers *o, const sfe_icp_dpf *rd,
                                     int n_rd, const sfe_icp_dpf *rf, int n_rf, sfe_cloud_store3 *s, const int32_t *pairs,
                                     const float *guesses16, int n_jobs, float *T_out16, int32_t *status, int32_t *iters)
{
    if (int rc = s3_check(ctx, s))
        return rc;
    if (int rc = sfe_icp3_check_params(ctx, p))
        return rc;
    if (int rc = sfe_icp3_check_chain(ctx, o, rd, n_rd, rf, n_rf))
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
    return sfe_icp3_chain_run_dev(ctx, p, o, rd, n_rd, rf, n_rf, s->d_pool, s->d_pool, jobs4.data(), guesses16, n_jobs, T_out16,
                                  status, iters);
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
