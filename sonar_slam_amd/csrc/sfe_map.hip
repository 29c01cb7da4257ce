// Log-odds occupancy map of bruce_slam's mapping.py (method 1) on the device: the polar measurement image of a keyframe,
// the fit of its pixels to grid cells, and the ordered add / subtract of its cells on a float32 grid (sonar_slam_amd/mapping.py
// is the host side: control flow, growth decisions, everything O(keyframes)).
//
// One implementation, sfe_mapset: S maps that advance together.  Every kernel runs over (map, slot) jobs whose tables carry
// pointers, so a job does not know which map it belongs to.  State of a map: the grid [rows x cols] float32; of the set: the
// sonar_xy table of every geometry, and per keyframe slot its polar log-odds image and its cell list (r, c uint16 +
// l float32, ascending r * cols + c).  Cell lists are double-buffered: a refit writes the new list next to the old one,
// subtracts the old, adds the new, and flips.  Growth pads a grid and bumps two counters; a list keeps the counters it was
// written at, and its cells are shifted by the difference when read.  An sfe_map is a set of one map (the end of this file).
// Method 2 (get_occupancy_grid2: point projection + dilation) reads those cell lists and writes no state: sfe_mapset_render2.
// The intensity mosaic (pub_intensity, mapping.py:241-243, 272-298, 442-444), only after sfe_mapset_enable_intensity: per
// slot the subsampled ping (uint8) and a fourth list payload i next to l; per map a uint32 sum grid and a uint16 counter grid
// of the float grid's shape, updated by the same applies and padded by the same growth; sfe_mapset_render_intensity.
//
// Slot storage, the one thing chosen at creation.  A slot record (SetSlot) carries its own device pointers:
//   logodds  float32 [px]
//   r, c     uint16  [2][px] each   (the double-buffered cell list)
//   l        float32 [2][px]
// = 20 bytes per pixel (2.1 MB at the 105 k pixels of a 1024 x 512 ping at the shipped skips), plus 8 bytes of counts.
// With the intensity mosaic enabled also
//   image    uint8   [px]           (the ping at the geometry's skips)
//   i        uint8   [2][px]
// = 23 bytes per pixel.
//   arena (sfe_mapset_create): fixed at creation for n_maps * max_keyframes slots of max_px pixels each, the pointers computed
//     into it then.  Nothing is reallocated afterwards: a slot >= max_keyframes or an image of more than max_px pixels is
//     refused (SFE_ERR_CAP) before any state changes.
//   on demand (sfe_map_create): no cap.  A slot's buffers are allocated at its geometry's pixel count when its measurement
//     (or set_logodds) runs, and the slot vector and the counts table grow to hold it, live counts kept.
// Everything else reads the pointers of the record.  Grids are per map and grow on their own.
#include <algorithm>
#include <climits>
#include <cstring>
#include <utility>

#include "sfe_internal.h"
#include "sfe_map_intensity.h"

namespace {

constexpr int MAP_THREADS = 256;
constexpr int COMPACT_THREADS = 1024;
constexpr int32_t EMPTY_SLOT = INT_MAX;

struct MapGeom {
    float2 *d_xy = nullptr;
    int img_rows = 0, img_cols = 0;
};

struct MapBuf {
    void *p = nullptr;
    size_t cap = 0;
};

struct SetSlot {
    int geom = -1;              // -1: unused
    int cur = 0;                // which buffer holds the current list
    int has_cells = 0;
    int base_r = 0, base_c = 0; // growth counters when the current list was written
    int px = 0;                 // pixels its buffers hold
    float *d_logodds = nullptr;
    uint16_t *d_r[2] = {nullptr, nullptr}, *d_c[2] = {nullptr, nullptr};
    float *d_l[2] = {nullptr, nullptr};
    int32_t *d_n = nullptr;     // [2]: cell count of each list buffer
    // the intensity mosaic (null unless enabled)
    int has_image = 0;
    uint8_t *d_image = nullptr, *d_i[2] = {nullptr, nullptr};
};

struct SetMap {
    int rows = 0, cols = 0;
    float *d_grid = nullptr, *d_frames = nullptr; // (d_frames: the grid of the last frames= render)
    int frames_rows = 0, frames_cols = 0;
    int grow_r = 0, grow_c = 0;
    uint32_t *d_inten = nullptr; // the intensity mosaic's sum and counter grids (null unless enabled)
    uint16_t *d_count = nullptr;
};

// per keyframe of a measurement batch
struct MeasJob {
    int32_t slot_px;   // pixels of its image
    int32_t img_rows, img_cols;
    int32_t hit_off, n_hits; // its hits in the batch's hit table
    int32_t hr, hc;    // kernel half sizes
    int32_t k_off;     // its float32 kernel in the batch's kernel table ((2hr+1) x (2hc+1), row-major)
    int64_t px_off;    // its pixels in the batch scratch (mask / probabilities)
    double div;        // kernel[hr, hc] / hit_prob (float64, mapping.py:212)
    float *logodds;    // the slot's image
};

// per keyframe of a fit batch
struct FitJob {
    const float2 *xy;
    int32_t n_px;
    double c, s, tx, ty;   // rotation and translation (host cos / sin of the pose's theta)
    double y0, x0;         // grid origin at the time of the fit
    int32_t wr0, wc0, wh, ww; // cell window = [wr0, wr0 + wh) x [wc0, wc0 + ww) in fit coordinates
    int32_t sr, sc;        // shift of the fitted cells into the grid's current coordinates
    int64_t win_off;       // its window in the slot scratch
    const float *logodds;
    uint16_t *out_r, *out_c;
    float *out_l;
    int32_t *out_n;
    const uint8_t *image; // the intensity mosaic's payload (null: none)
    uint8_t *out_i;
};

// per keyframe of an intensity upload: out[i * img_cols + j] = src[i * r_skip * stride + j * c_skip]
struct SampleJob {
    const uint8_t *src;
    uint8_t *out;
    int32_t img_rows, img_cols, r_skip, c_skip;
    int64_t stride;
};

struct FeedJob {
    long long off;
    int32_t n, hit_off, tab;
};
// what Mapping._hit_indices reads of a sonar geometry and its skips
struct HitTab {
    const double *breaks; // [n_iv + 1] ascending: the knots of oculus.b2c's cubic spline
    const double *coef;   // [n_iv][4]: its cubic on [breaks[k], breaks[k + 1]) in powers of (a - breaks[k]), highest first
    int32_t n_iv, num_ranges, num_bearings, r_skip, c_skip;
    int32_t wide;         // ra / range_resolution - 1 in float64 (a numpy float64 scalar resolution), else in float32
    float res32;
    double res64, b_first, b_last, margin;
};
struct UndPoint {
    float x, y;
    int32_t pos, job; // its entry in the hit buffer
};


// the store feed: the call that waits for the host's cells
struct FeedState {
    bool pending = false;
    std::vector<int32_t> maps, slots, geoms, n_und;
    std::vector<MeasJob> jobs;
    std::vector<float> ktab;
    float miss32 = 0, logit_miss = 0, hit32 = 0, logit_hit = 0;
    int tot = 0, tot_und = 0;
};

} // namespace

struct sfe_mapset {
    sfe_ctx *ctx = nullptr;
    bool arena = true;  // slot storage: the fixed arena, or on demand
    int n_maps = 0;
    int max_kf = 0;     // slots per map: fixed (arena), or as many as have been asked for (on demand)
    int max_px = 0;     // (arena)
    std::vector<SetMap> maps;
    std::vector<MapGeom> geoms;
    std::vector<SetSlot> slots; // [map * max_kf + slot]
    float *d_logodds = nullptr, *d_l = nullptr; // the arena
    uint16_t *d_r = nullptr, *d_c = nullptr;
    bool intensity = false;               // sfe_mapset_enable_intensity
    uint8_t *d_image = nullptr, *d_i = nullptr; // its part of the arena
    int32_t *d_counts = nullptr; // [map * max_kf + slot][2], room for counts_cap slots
    int counts_cap = 0;
    // scratch.  0 .. 5: job tables, hits, kernels, mask, image, first hits; 6 .. 10: the store feed's job tables, hit buffer,
    // keep flags, undecided lists and counters, hit tables; 11 .. 16: method 2's job tables, list table, spans, points,
    // float32 points + keep flags, work images; 17, 18: its store route's frame lists, multiplicities + keep flags;
    // 19, 20: the intensity upload's job table and full-size images
    MapBuf buf[21];
    int last_meas_n = 0;
    std::vector<MeasJob> last_meas;
    long long apply_launches = 0; // launches of mapset_apply_kernel so far
    std::vector<HitTab> hit_tabs; // device copies owned here
    FeedState feed;
};

namespace {

// grow-only device scratch
void *buf_get(sfe_ctx *ctx, MapBuf &b, size_t bytes)
{
    if (b.cap >= bytes && b.p)
        return b.p;
    if (b.p) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(b.p);
        b.p = nullptr;
        b.cap = 0;
    }
    size_t cap = bytes + bytes / 4 + 256;
    if (hipMalloc(&b.p, cap) != hipSuccess) {
        b.p = nullptr;
        return nullptr;
    }
    b.cap = cap;
    return b.p;
}

// n values from pageable host memory (the caller synchronises before the host array goes away)
template <class T>
T *buf_upload(sfe_ctx *ctx, MapBuf &b, const T *h, size_t n)
{
    T *d = (T *)buf_get(ctx, b, sizeof(T) * (n ? n : 1));
    if (!d)
        return nullptr;
    if (n && hipMemcpyAsync(d, h, sizeof(T) * n, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        return nullptr;
    return d;
}

// a job table through pinned staging: enqueue only
template <class T>
T *buf_stage(sfe_ctx *ctx, MapBuf &b, const std::vector<T> &jobs)
{
    const size_t bytes = sizeof(T) * jobs.size();
    T *d = (T *)buf_get(ctx, b, bytes ? bytes : 1);
    if (!d || !bytes)
        return d;
    void *pin = sfe_pinned_begin(ctx, bytes);
    if (!pin)
        return nullptr;
    memcpy(pin, jobs.data(), bytes);
    if (hipMemcpyAsync(d, pin, bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        return nullptr;
    if (sfe_pinned_end(ctx, ctx->stream))
        return nullptr;
    return d;
}

// --- measurement (mapping.py:170-228) ---------------------------------------------------------------------------------
__global__ void map_hits_kernel(const MeasJob *jobs, const int32_t *hits, uint8_t *mask)
{
    const MeasJob j = jobs[blockIdx.y];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < j.n_hits; i += gridDim.x * blockDim.x) {
        const int r = hits[2 * (j.hit_off + i)], c = hits[2 * (j.hit_off + i) + 1];
        if (r >= 0 && r < j.img_rows && c >= 0 && c < j.img_cols)
            mask[j.px_off + (int64_t)r * j.img_cols + c] = 1;
    }
}

// cv2.filter2D(mask, CV_32F, kernel, BORDER_CONSTANT) as a direct sum in the kernel's row-major order: the image holds 0 and 1,
// so only the hits inside the window add (their coefficient, exactly), in that order; then / div in float64 and the clip.
__global__ void map_filter_kernel(const MeasJob *jobs, const float *ktab, const uint8_t *mask, float *prob, float hit32)
{
    const MeasJob j = jobs[blockIdx.y];
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= j.slot_px)
        return;
    const int y = p / j.img_cols, x = p - y * j.img_cols;
    const int kw = 2 * j.hc + 1;
    const uint8_t *m = mask + j.px_off;
    const float *k = ktab + j.k_off;
    float s = 0.0f;
    for (int i = 0; i <= 2 * j.hr; ++i) {
        const int yy = y + i - j.hr;
        if (yy < 0 || yy >= j.img_rows)
            continue;
        for (int jj = 0; jj < kw; ++jj) {
            const int xx = x + jj - j.hc;
            if (xx >= 0 && xx < j.img_cols && m[(int64_t)yy * j.img_cols + xx])
                s = __fadd_rn(s, k[i * kw + jj]);
        }
    }
    float v = (float)__ddiv_rn((double)s, j.div);
    v = v < 0.5f ? 0.5f : v;     // np.clip(mask, 0.5, hit_prob) = minimum(maximum(mask, 0.5), hit_prob)
    v = v > hit32 ? hit32 : v;
    prob[j.px_off + p] = v;
}

__device__ __forceinline__ float map_logit(float v, float miss32, float logit_miss, float hit32, float logit_hit)
{
    if (v == miss32)
        return logit_miss;
    if (v == hit32)
        return logit_hit;
    const double d = (double)v;
    return (float)log(__ddiv_rn(d, __dsub_rn(1.0, d)));
}

// per column: the first row > 0.5 (np.argmax; 0 for no hit and for a hit in row 0 alike, and then the whole column is a miss),
// the rows above it set to miss_prob, then logit.  A keyframe without points (hr < 0) is all miss_prob.
__global__ void map_columns_kernel(const MeasJob *jobs, float *prob, int32_t *first_hits, float miss32, float logit_miss,
                                   float hit32, float logit_hit, int64_t fh_stride)
{
    const MeasJob j = jobs[blockIdx.y];
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= j.img_cols)
        return;
    float *pc = prob + j.px_off + col;
    int fh = j.img_rows;
    if (j.hr >= 0) {
        fh = 0;
        for (int r = 0; r < j.img_rows; ++r)
            if (pc[(int64_t)r * j.img_cols] > 0.5f) {
                fh = r;
                break;
            }
        if (fh == 0)
            fh = j.img_rows;
    }
    first_hits[blockIdx.y * fh_stride + col] = fh;
    for (int r = 0; r < j.img_rows; ++r) {
        const int64_t o = (int64_t)r * j.img_cols;
        float v = r < fh ? miss32 : pc[o];
        pc[o] = v;
        j.logodds[o + col] = map_logit(v, miss32, logit_miss, hit32, logit_hit);
    }
}

// --- fit (mapping.py:466-499) -----------------------------------------------------------------------------------------
// xy = R.dot(sonar_xy.T).T + t in float64: this image's dgemm accumulates over k with a fused multiply-add,
// fma(R[i][1], y, fl(R[i][0] * x)), then the translation is added (pinned by tests/golden/mapping_session.npz); then
// round((v - origin) / resolution) half to even.
__device__ __forceinline__ void map_cell(const FitJob &j, float2 p, double res, int &r, int &c)
{
    const double X = (double)p.x, Y = (double)p.y;
    const double gx = __dadd_rn(__fma_rn(-j.s, Y, __dmul_rn(j.c, X)), j.tx);
    const double gy = __dadd_rn(__fma_rn(j.c, Y, __dmul_rn(j.s, X)), j.ty);
    r = (int)rint(__ddiv_rn(__dsub_rn(gy, j.y0), res));
    c = (int)rint(__ddiv_rn(__dsub_rn(gx, j.x0), res));
}

__device__ __forceinline__ int wave_min(int v)
{
    for (int o = 32; o > 0; o >>= 1)
        v = min(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ int wave_max(int v)
{
    for (int o = 32; o > 0; o >>= 1)
        v = max(v, __shfl_xor(v, o));
    return v;
}

// per keyframe: min / max of r and c over its pixels -> mm[4 b .. 4 b + 3] (initialised to INT_MAX / INT_MIN by the host)
__global__ void map_bounds_kernel(const FitJob *jobs, double res, int32_t *mm)
{
    const FitJob j = jobs[blockIdx.y];
    int rlo = INT_MAX, rhi = INT_MIN, clo = INT_MAX, chi = INT_MIN;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < j.n_px; p += gridDim.x * blockDim.x) {
        int r, c;
        map_cell(j, j.xy[p], res, r, c);
        rlo = min(rlo, r), rhi = max(rhi, r), clo = min(clo, c), chi = max(chi, c);
    }
    rlo = wave_min(rlo), rhi = wave_max(rhi), clo = wave_min(clo), chi = wave_max(chi);
    if ((threadIdx.x & 63) == 0 && rlo != INT_MAX) {
        int32_t *o = mm + 4 * blockIdx.y;
        atomicMin(o + 0, rlo);
        atomicMax(o + 1, rhi);
        atomicMin(o + 2, clo);
        atomicMax(o + 3, chi);
    }
}

// np.unique(r * cols + c, return_index=True): the first pixel of every cell.  The window of a 30 m fan at 0.2 m is up to about
// 300 x 300 cells, more than 160 KB of LDS holds as 32-bit slots, so it lives in HBM: one int per cell, the smallest pixel
// index wins (integer atomicMin: the same winner whatever the order).
__global__ void map_scatter_kernel(const FitJob *jobs, double res, int32_t *win)
{
    const FitJob j = jobs[blockIdx.y];
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= j.n_px)
        return;
    int r, c;
    map_cell(j, j.xy[p], res, r, c);
    r -= j.wr0, c -= j.wc0;
    if (r < 0 || r >= j.wh || c < 0 || c >= j.ww)
        return;   // cannot happen: the window is the bounds of these same cells
    atomicMin(win + j.win_off + (int64_t)r * j.ww + c, p);
}

// one workgroup per keyframe walks its window in row-major order (= ascending r * cols + c) and writes the occupied cells
__global__ __launch_bounds__(COMPACT_THREADS) void map_compact_kernel(const FitJob *jobs, const int32_t *win)
{
    __shared__ int wave_tot[COMPACT_THREADS / 64];
    __shared__ int carry_s;
    const FitJob j = jobs[blockIdx.x];
    const int64_t n = (int64_t)j.wh * j.ww;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int64_t base = 0; base < n; base += COMPACT_THREADS) {
        const int64_t i = base + threadIdx.x;
        const int32_t v = i < n ? win[j.win_off + i] : EMPTY_SLOT;
        const bool on = v != EMPTY_SLOT;
        const unsigned long long bal = __ballot(on);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0)
            wave_tot[wave] = __popcll(bal);
        __syncthreads();
        int off = carry;
        int tot = 0;
        for (int w = 0; w < COMPACT_THREADS / 64; ++w) {
            off += w < wave ? wave_tot[w] : 0;
            tot += wave_tot[w];
        }
        if (on && v >= 0 && v < j.n_px) {
            const int k = off + before;
            const int rr = (int)(i / j.ww), cc = (int)(i - (int64_t)rr * j.ww);
            j.out_r[k] = (uint16_t)(j.wr0 + rr + j.sr);
            j.out_c[k] = (uint16_t)(j.wc0 + cc + j.sc);
            j.out_l[k] = j.logodds[v];
            if (j.out_i)
                j.out_i[k] = j.image[v];
        }
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        carry_s = carry;
        *j.out_n = carry_s;
    }
}

template <class T>
__global__ void map_pad_kernel(const T *src, int rows, int cols, T *dst, int dcols, int top, int left)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)rows * cols)
        return;
    const int r = (int)(i / cols), c = (int)(i - (int64_t)r * cols);
    dst[(int64_t)(r + top) * dcols + c + left] = src[i];
}

// r2n(ping.ping)[::r_skip, ::c_skip] (mapping.py:242) of job blockIdx.y: consecutive threads take consecutive columns of a
// row, so with c_skip == 1 a wave reads and writes whole runs of bytes; with c_skip > 1 it reads every c_skip-th byte of
// the same lines
__global__ __launch_bounds__(MAP_THREADS) void map_sample_kernel(const SampleJob *jobs)
{
    const SampleJob j = jobs[blockIdx.y];
    const int n = j.img_rows * j.img_cols;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        const int y = p / j.img_cols, x = p - y * j.img_cols;
        j.out[p] = j.src[(int64_t)y * j.r_skip * j.stride + (int64_t)x * j.c_skip];
    }
}

// --- apply (inc_grid / dec_grid) and render (get_occupancy_grid1) over job tables: one job serves one map as well as S ---
// one ordered add / subtract of a cell list on its map's grid
struct ApplyJob {
    float *grid;
    int32_t rows, cols;
    const uint16_t *r, *c;
    const float *l;
    const int32_t *n;
    int32_t dr, dc; // growth since the list was written
    int32_t sub;
    int32_t n_px; // upper bound of *n (the pixels of its image)
    // the intensity mosaic rides along (null: none): grid_i[cell] += / -= i, grid_n[cell] += / -= 1, wrapping
    uint32_t *grid_i;
    uint16_t *grid_n;
    const uint8_t *i;
};

struct RenderIJob {
    const uint32_t *grid_i;
    const uint16_t *grid_n;
    int32_t cols, r0, c0, h, w;
    int64_t out_off;
};

struct RenderJob {
    const float *grid;
    int32_t cols, r0, c0, h, w, oh, ow, resize;
    double inv;
    int64_t out_off;
};

// One round: job blockIdx.y is the next apply of one map, so no two jobs of a launch share a grid, and the cells of a list are
// unique: plain loads and stores, every cell written by one thread.  One pass, 8 B read + 4 B read-modify-write per cell.
__global__ __launch_bounds__(MAP_THREADS) void mapset_apply_kernel(const ApplyJob *jobs)
{
    const ApplyJob j = jobs[blockIdx.y];
    const int n = min(*j.n, j.n_px);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int rr = (int)j.r[i] + j.dr, cc = (int)j.c[i] + j.dc;
        if (rr < 0 || rr >= j.rows || cc < 0 || cc >= j.cols)
            continue; // cannot happen: every cell lies inside the grown grid
        const int64_t cell = (int64_t)rr * j.cols + cc;
        float *g = j.grid + cell;
        *g = j.sub ? __fsub_rn(*g, j.l[i]) : __fadd_rn(*g, j.l[i]);
        if (j.grid_i) {
            // the counter's neighbours in its dword belong to other lanes: a 16-bit load and a 16-bit store, nothing wider
            uint32_t *gi = j.grid_i + cell;
            uint16_t *gn = j.grid_n + cell;
            const uint32_t v = j.i[i];
            *gi = j.sub ? *gi - v : *gi + v;
            *gn = (uint16_t)(j.sub ? *gn - 1u : *gn + 1u);
        }
    }
}

// get_intensity_grid (mapping.py:272-298): job blockIdx.y writes its h x w box at out + out_off
__global__ __launch_bounds__(MAP_THREADS) void mapset_render_intensity_kernel(const RenderIJob *jobs, int8_t *out)
{
    const RenderIJob j = jobs[blockIdx.y];
    const int64_t n = (int64_t)j.h * j.w;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(i / j.w), x = (int)(i - (int64_t)y * j.w);
        const int64_t cell = (int64_t)(j.r0 + y) * j.cols + j.c0 + x;
        out[j.out_off + i] = sfe_map_intensity_value(j.grid_i[cell], j.grid_n[cell]);
    }
}

// get_occupancy_grid1 (mapping.py:306-355): crop, expit, INTER_NEAREST, int8(clip(100 p, 0, 100)); job blockIdx.y writes its
// out_h x out_w image at out + out_off
__global__ __launch_bounds__(MAP_THREADS) void mapset_render_kernel(const RenderJob *jobs, int8_t *out)
{
    const RenderJob j = jobs[blockIdx.y];
    const int64_t n = (int64_t)j.oh * j.ow;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(i / j.ow), x = (int)(i - (int64_t)y * j.ow);
        int sy = y, sx = x;
        if (j.resize) {
            sy = min((int)floor(__dmul_rn((double)y, j.inv)), j.h - 1);
            sx = min((int)floor(__dmul_rn((double)x, j.inv)), j.w - 1);
        }
        const double v = (double)j.grid[(int64_t)(j.r0 + sy) * j.cols + j.c0 + sx];
        const float p = (float)__ddiv_rn(1.0, __dadd_rn(1.0, exp(-v)));
        float q = __fmul_rn(100.0f, p);
        q = q < 0.0f ? 0.0f : (q > 100.0f ? 100.0f : q);
        out[j.out_off + i] = (int8_t)(int)q;
    }
}

// pcl.remove_outlier's decision (radius_count_kernel of sfe_icp.hip, the same float32 arithmetic) for one cloud of a launch
// over many: block blockIdx.x of the cloud's row; keep iff more than min_points points (itself included) lie within the radius
__device__ __forceinline__ void radius_count_cloud(const float2 *__restrict__ cloud, int n, float r2, int min_points,
                                                   uint8_t *__restrict__ keep, float2 *s_p /* [2048], shared */)
{
    if ((int)(blockIdx.x * 256) >= n)
        return; // the whole block at once
    const int i = blockIdx.x * 256 + threadIdx.x;
    float px = 0, py = 0;
    if (i < n) {
        const float2 p = cloud[i];
        px = p.x;
        py = p.y;
    }
    int cnt = 0;
    for (int tb = 0; tb < n; tb += 2048) {
        const int tn = min(2048, n - tb);
        __syncthreads();
        for (int j = threadIdx.x; j < tn; j += 256)
            s_p[j] = cloud[tb + j];
        __syncthreads();
        for (int j = 0; j < tn; ++j) {
            const float2 t = s_p[j];
            const float dx = __fadd_rn(px, -t.x), dy = __fadd_rn(py, -t.y);
            cnt += __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)) <= r2;
        }
    }
    if (i < n)
        keep[i] = cnt > min_points;
}

// ... cloud blockIdx.y = pts[off[y] .. off[y + 1])
__global__ __launch_bounds__(256) void radius_count_many_kernel(const float2 *__restrict__ pts, const int32_t *__restrict__ off,
                                                                float r2, int min_points, uint8_t *__restrict__ keep)
{
    __shared__ float2 s_p[2048];
    const int base = off[blockIdx.y];
    radius_count_cloud(pts + base, off[blockIdx.y + 1] - base, r2, min_points, keep + base, s_p);
}

// --- method 2 (get_occupancy_grid2, mapping.py:357-439) over job tables: one job = one published image --------------------
// Its work image is the known region, h x w int8, at work + work_off: -1 everywhere, 0 where a listed keyframe has a cell,
// 100 under the ellipse element of every kept point that projects into the region; then INTER_NEAREST into the packed output.
// The launches follow each other on the context's stream, which keeps 100 above 0; (b) and (d) store a constant, so equal
// stores from several threads need no ordering.
struct Render2Job {
    int32_t h, w, oh, ow, resize;
    int32_t pt_off, n_pts; // its points in the call's point table
    int32_t filter;        // the radius filter runs: the projection then reads the float32-rounded point
    int32_t min_points;
    float r2;
    int32_t hs, span_off;  // half size of the element; its row spans in the call's span table
    double y0, x0, res;    // the region's corner in metres, the map's resolution
    double inv;
    int64_t work_off, out_off;
    // the store route (sfe_mapset_render2_store): its cloud in the store's pool, its frame list in the call's list table
    int64_t pool_off;
    int32_t frame_off, n_frames; // n_frames < 0: all frames
};

// the current cell list of one listed keyframe of a job
struct MarkJob {
    int8_t *img;
    int32_t h, w;
    const uint16_t *r, *c;
    const int32_t *n;
    int32_t dr, dc; // growth since the list was written, less the region's corner
    int32_t n_px;   // upper bound of *n
};

// (a) every work image of the call starts unknown: they lie back to back, n16 16-byte words in all
__global__ __launch_bounds__(MAP_THREADS) void map2_fill_kernel(uint4 *work, int64_t n16)
{
    const uint4 unknown = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (int64_t)gridDim.x * blockDim.x)
        work[i] = unknown;
}

// (b) occ[keyframe.r - rmin, keyframe.c - cmin] = 0: list blockIdx.y, shifted as mapset_apply_kernel shifts it
__global__ __launch_bounds__(MAP_THREADS) void map2_mark_kernel(const MarkJob *jobs)
{
    const MarkJob j = jobs[blockIdx.y];
    const int n = min(*j.n, j.n_px);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int rr = (int)j.r[i] + j.dr, cc = (int)j.c[i] + j.dc;
        if (rr < 0 || rr >= j.h || cc < 0 || cc >= j.w)
            continue; // cannot happen: the region is the union of the listed keyframes' boxes
        j.img[(int64_t)rr * j.w + cc] = 0;
    }
}

// (c) the points as pybind hands them to pcl.remove_outlier (float32), every point kept until the filter says otherwise
__global__ __launch_bounds__(MAP_THREADS) void map2_cast_kernel(const double2 *__restrict__ xy, int n, float2 *__restrict__ xy32,
                                                                uint8_t *__restrict__ keep)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const double2 p = xy[i];
    xy32[i] = make_float2((float)p.x, (float)p.y);
    keep[i] = 1;
}

// ... and the filter's decision for the jobs that run it: job blockIdx.y, block blockIdx.x of its cloud's row
__global__ __launch_bounds__(256) void map2_radius_count_kernel(const Render2Job *__restrict__ jobs, const float2 *__restrict__ xy32,
                                                                uint8_t *__restrict__ keep)
{
    __shared__ float2 s_p[2048];
    const int32_t filter = jobs[blockIdx.y].filter, off = jobs[blockIdx.y].pt_off, n = jobs[blockIdx.y].n_pts;
    if (!filter)
        return; // the whole block at once
    radius_count_cloud(xy32 + off, n, jobs[blockIdx.y].r2, jobs[blockIdx.y].min_points, keep + off, s_p);
}

// (c') the store route's points stay where they are, float32 in the store's pool; what mapping.py:365-372 makes of them is a
// multiset: point i is taken once for every entry of the job's frame list that equals its key (a key listed twice gives its
// rows twice, an entry no point carries gives nothing; keys are >= 0, so a negative entry is such an entry).  mult[i] is
// that multiplicity, 1 for every point of a job that takes all frames; keep[i] = mult[i] > 0 until the filter says otherwise.
// Job blockIdx.y, block blockIdx.x of its cloud's row; the list goes through LDS in tiles of 1024 entries.
__global__ __launch_bounds__(256) void map2_select_kernel(const Render2Job *__restrict__ jobs, const int32_t *__restrict__ key_pool,
                                                          const int32_t *__restrict__ frames, int32_t *__restrict__ mult,
                                                          uint8_t *__restrict__ keep)
{
    __shared__ int32_t s_f[1024];
    const int32_t n = jobs[blockIdx.y].n_pts, off = jobs[blockIdx.y].pt_off, nf = jobs[blockIdx.y].n_frames;
    if ((int)(blockIdx.x * 256) >= n)
        return; // the whole block at once
    const int i = blockIdx.x * 256 + threadIdx.x;
    int m = 1;
    if (nf >= 0) {
        const int32_t *list = frames + jobs[blockIdx.y].frame_off;
        const int32_t key = i < n ? key_pool[jobs[blockIdx.y].pool_off + i] : -1;
        m = 0;
        for (int tb = 0; tb < nf; tb += 1024) {
            const int tn = min(1024, nf - tb);
            __syncthreads();
            for (int j = threadIdx.x; j < tn; j += 256)
                s_f[j] = list[tb + j];
            __syncthreads();
            for (int j = 0; j < tn; ++j)
                m += s_f[j] == key;
        }
    }
    if (i < n) {
        mult[off + i] = m;
        keep[off + i] = m > 0;
    }
}

// ... and radius_count_cloud's decision over that multiset: every neighbour counts mult times (a point's own copies too), so
// a selected point stays iff the host's count over the repeated rows would keep its copies
__global__ __launch_bounds__(256) void map2_radius_count_store_kernel(const Render2Job *__restrict__ jobs,
                                                                      const float2 *__restrict__ pool,
                                                                      const int32_t *__restrict__ mult, uint8_t *__restrict__ keep)
{
    __shared__ float2 s_p[2048];
    __shared__ int32_t s_m[2048];
    const Render2Job &jb = jobs[blockIdx.y];
    const int32_t n = jb.n_pts, off = jb.pt_off, min_points = jb.min_points;
    const float r2 = jb.r2;
    if (!jb.filter || (int)(blockIdx.x * 256) >= n)
        return; // the whole block at once
    const float2 *cloud = pool + jb.pool_off;
    const int i = blockIdx.x * 256 + threadIdx.x;
    float px = 0, py = 0;
    if (i < n) {
        const float2 p = cloud[i];
        px = p.x;
        py = p.y;
    }
    long long cnt = 0;
    for (int tb = 0; tb < n; tb += 2048) {
        const int tn = min(2048, n - tb);
        __syncthreads();
        for (int j = threadIdx.x; j < tn; j += 256) {
            s_p[j] = cloud[tb + j];
            s_m[j] = mult[off + tb + j];
        }
        __syncthreads();
        for (int j = 0; j < tn; ++j) {
            const float2 t = s_p[j];
            const float dx = __fadd_rn(px, -t.x), dy = __fadd_rn(py, -t.y);
            cnt += __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)) <= r2 ? s_m[j] : 0;
        }
    }
    if (i < n)
        keep[off + i] = mult[off + i] > 0 && cnt > (long long)min_points;
}

// (d) r = int32(round((y - y0) / resolution)), c likewise, in double (y0 is a numpy float64 scalar, so numpy widens a
// float32 cloud): one IEEE subtract, one divide, round half to even.  A point outside the region is dropped; one inside is
// dilated by the element, clipped at the region's border (cv2.dilate's constant border).  One thread per (point, element
// row): it stores the row's span.  With `pool` (the store route) the point is the float32 one of the job's cloud there.
__global__ __launch_bounds__(MAP_THREADS) void map2_stamp_kernel(const Render2Job *__restrict__ jobs,
                                                                 const double2 *__restrict__ xy, const float2 *__restrict__ xy32,
                                                                 const float2 *__restrict__ pool, const uint8_t *__restrict__ keep,
                                                                 const int32_t *__restrict__ spans, int8_t *work)
{
    const Render2Job j = jobs[blockIdx.y];
    const int size = 2 * j.hs + 1;
    const int64_t n = (int64_t)j.n_pts * size;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const int p = (int)(t / size), i = (int)(t - (int64_t)p * size);
        const int q = j.pt_off + p;
        if (!keep[q])
            continue;
        double x, y;
        if (pool) {
            const float2 f = pool[j.pool_off + p];
            x = (double)f.x, y = (double)f.y;
        } else if (j.filter) {
            const float2 f = xy32[q];
            x = (double)f.x, y = (double)f.y;
        } else {
            const double2 d = xy[q];
            x = d.x, y = d.y;
        }
        const double fr = rint(__ddiv_rn(__dsub_rn(y, j.y0), j.res)), fc = rint(__ddiv_rn(__dsub_rn(x, j.x0), j.res));
        if (!(fr >= 0.0 && fr < (double)j.h && fc >= 0.0 && fc < (double)j.w))
            continue; // (a NaN too)
        const int rr = (int)fr + i - j.hs;
        if (rr < 0 || rr >= j.h)
            continue;
        const int left = (int)fc - j.hs;
        const int c0 = max(left + spans[j.span_off + 2 * i], 0), c1 = min(left + spans[j.span_off + 2 * i + 1], j.w);
        int8_t *row = work + j.work_off + (int64_t)rr * j.w;
        for (int cc = c0; cc < c1; ++cc)
            row[cc] = 100;
    }
}

// (e) cv2.resize(occ, None, None, ratio, ratio, INTER_NEAREST), or the copy: mapset_render_kernel's index rule
__global__ __launch_bounds__(MAP_THREADS) void map2_resize_kernel(const Render2Job *__restrict__ jobs,
                                                                  const int8_t *__restrict__ work, int8_t *__restrict__ out)
{
    const Render2Job j = jobs[blockIdx.y];
    const int64_t n = (int64_t)j.oh * j.ow;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int y = (int)(i / j.ow), x = (int)(i - (int64_t)y * j.ow);
        int sy = y, sx = x;
        if (j.resize) {
            sy = min((int)floor(__dmul_rn((double)y, j.inv)), j.h - 1);
            sx = min((int)floor(__dmul_rn((double)x, j.inv)), j.w - 1);
        }
        out[j.out_off + i] = work[j.work_off + (int64_t)sy * j.w + sx];
    }
}

// --- the store feed: a keyframe's hits straight from its cloud in a cloud store (mapping.py: MapBatch.add_keyframes_store) ----
// One job = one cloud (pool offset, size) for one (map, slot); its points own the entries [hit_off, hit_off + n) of the call's
// hit buffer, one (row, column) pair per point, (-1, -1) for a point that leaves no hit (map_hits_kernel skips those).
// the outlier filter of every job's cloud: keep[hit_off + i]
__global__ __launch_bounds__(256) void feed_radius_count_kernel(const float2 *__restrict__ pool, const FeedJob *__restrict__ jobs,
                                                                float r2, int min_points, uint8_t *__restrict__ keep)
{
    __shared__ float2 s_p[2048];
    const FeedJob j = jobs[blockIdx.y];
    radius_count_cloud(pool + j.off, j.n, r2, min_points, keep + j.hit_off, s_p);
}

// Mapping._hit_indices for the kept float32 points of every job (numpy 2 promotion):
//   r = clip(int32(round(norm(p) / range_resolution - 1)), 0, num_ranges - 1) // r_skip
//   c = clip(int32(round(b2c(arctan2(y, x)))), 0, num_bearings - 1) // c_skip
// The row is exact: float32 multiply, add, the correctly rounded sqrtf (see store_fov_kernel), divide, subtract, rint.
// The column is not reproduced to the last bit: numpy takes atan2f in float32 and scipy evaluates the B-spline in double;
// here atan2 is taken in double and the spline as one cubic per knot interval (PPoly coefficients from the host).  With
// a = the true angle, numpy's a32 = atan2f(y, x) lies within one float32 ulp u of it (u taken at max(1, largest |bearing|),
// no smaller than the ulp of any angle inside the table), the double atan2 within 1e-15.  So the column numpy rounds lies
// within u * slope + (the two evaluations' own difference, some 1e-12 columns) of the one computed here, where slope is
// the largest |d column / d angle| of the table (no less than 1, so that the same number also bounds u itself).  The host
// passes margin = 2 * u * slope + 1e-9.  A point is decided only if its column value is further than margin from every
// rounding boundary x.5, and its angle either further than margin inside both table ends or further than margin outside
// one (outside: fill_value -1, which clips to column 0).  Every other point goes to its job's undecided list; the host
// runs _hit_indices on just those.
__global__ __launch_bounds__(256) void feed_hit_cells_kernel(const float2 *__restrict__ pool, const FeedJob *__restrict__ jobs,
                                                             const HitTab *__restrict__ tabs, const uint8_t *__restrict__ keep,
                                                             int32_t *__restrict__ hits, UndPoint *__restrict__ und,
                                                             int32_t *__restrict__ n_und)
{
    const int jb = blockIdx.y;
    const FeedJob j = jobs[jb];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= j.n)
        return;
    const int pos = j.hit_off + i;
    int hr = -1, hc = -1;
    if (!keep || keep[pos]) {
        const float2 p = pool[j.off + i];
        const HitTab t = tabs[j.tab];
        const float ra = sqrtf(__fadd_rn(__fmul_rn(p.x, p.x), __fmul_rn(p.y, p.y)));
        int ri = INT_MIN; // what np.int32 makes of a value no int32 holds (and of nan)
        if (t.wide) {
            const double ro = rint(__dsub_rn(__ddiv_rn((double)ra, t.res64), 1.0));
            if (ro >= -2147483648.0 && ro < 2147483648.0)
                ri = (int)ro;
        } else {
            const float ro = rintf(__fsub_rn(__fdiv_rn(ra, t.res32), 1.0f));
            if (ro >= -2147483648.0f && ro < 2147483648.0f)
                ri = (int)ro;
        }
        ri = min(max(ri, 0), t.num_ranges - 1);
        const double a = atan2((double)p.y, (double)p.x);
        bool decided = false;
        int col = 0;
        if (a < t.b_first - t.margin || a > t.b_last + t.margin) {
            decided = true;
        } else if (a > t.b_first + t.margin && a < t.b_last - t.margin) {
            int lo = 0, hi = t.n_iv; // breaks[lo] <= a < breaks[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (t.breaks[mid] <= a)
                    lo = mid;
                else
                    hi = mid;
            }
            const double d = a - t.breaks[lo];
            const double *c = t.coef + 4 * lo;
            const double v = ((c[0] * d + c[1]) * d + c[2]) * d + c[3];
            if (fabs(v) < 1e9) {
                decided = fabs(v - floor(v) - 0.5) > t.margin;
                col = min(max((int)rint(v), 0), t.num_bearings - 1);
            }
        }
        if (decided) {
            hr = ri / t.r_skip;
            hc = col / t.c_skip;
        } else {
            const int k = atomicAdd(&n_und[jb], 1);
            UndPoint u;
            u.x = p.x, u.y = p.y, u.pos = pos, u.job = jb;
            und[j.hit_off + k] = u; // at most n entries per job
        }
    }
    hits[2 * pos] = hr;
    hits[2 * pos + 1] = hc;
}

// the host's cells of the undecided points
__global__ void feed_fill_kernel(const int32_t *__restrict__ pos, const int32_t *__restrict__ cells, int n,
                                 int32_t *__restrict__ hits)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        hits[2 * pos[i]] = cells[2 * i];
        hits[2 * pos[i] + 1] = cells[2 * i + 1];
    }
}


inline size_t set_idx(const sfe_mapset *ms, int map, int slot) { return (size_t)map * ms->max_kf + slot; }

int set_grid_alloc(sfe_mapset *ms, float **d, size_t n)
{
    if (hipMalloc((void **)d, n * sizeof(float)) != hipSuccess)
        return sfe_set_err(ms->ctx, SFE_ERR_HIP, "map set grid allocation of %zu cells failed", n);
    SFE_HIP(ms->ctx, hipMemsetAsync(*d, 0, n * sizeof(float), ms->ctx->stream));
    return 0;
}

// the intensity mosaic's two grids of one map, zeroed
int set_mosaic_alloc(sfe_mapset *ms, uint32_t **gi, uint16_t **gn, size_t n)
{
    *gi = nullptr, *gn = nullptr;
    if (hipMalloc((void **)gi, n * sizeof(uint32_t)) != hipSuccess || hipMalloc((void **)gn, n * sizeof(uint16_t)) != hipSuccess) {
        (void)hipFree(*gi);
        *gi = nullptr, *gn = nullptr;
        return sfe_set_err(ms->ctx, SFE_ERR_HIP, "map set intensity grid allocation of %zu cells failed", n);
    }
    SFE_HIP(ms->ctx, hipMemsetAsync(*gi, 0, n * sizeof(uint32_t), ms->ctx->stream));
    SFE_HIP(ms->ctx, hipMemsetAsync(*gn, 0, n * sizeof(uint16_t), ms->ctx->stream));
    return 0;
}

// may (map, slot) take an image of geometry g?  Checks only.
int set_slot_check(sfe_mapset *ms, int map, int slot, int g)
{
    sfe_ctx *ctx = ms->ctx;
    SFE_ARG(ctx, map >= 0 && map < ms->n_maps && slot >= 0 && g >= 0 && g < (int)ms->geoms.size());
    if (slot >= ms->max_kf) {
        if (!ms->arena)
            return 0; // set_slot_bind makes room
        return sfe_set_err(ctx, SFE_ERR_CAP, "map set: keyframe slot %d of map %d, room for %d keyframes per map", slot, map,
                           ms->max_kf);
    }
    const SetSlot &s = ms->slots[set_idx(ms, map, slot)];
    SFE_ARG(ctx, s.geom < 0 || s.geom == g);
    return 0;
}

// a used (map, slot)
int set_slot_used(sfe_mapset *ms, int map, int slot)
{
    SFE_ARG(ms->ctx, map >= 0 && map < ms->n_maps && slot >= 0 && slot < ms->max_kf &&
                         ms->slots[set_idx(ms, map, slot)].geom >= 0);
    return 0;
}

void set_slot_free(SetSlot &s)
{
    (void)hipFree(s.d_logodds);
    s.d_logodds = nullptr;
    for (int b = 0; b < 2; ++b) {
        (void)hipFree(s.d_r[b]);
        (void)hipFree(s.d_c[b]);
        (void)hipFree(s.d_l[b]);
        (void)hipFree(s.d_i[b]);
        s.d_r[b] = s.d_c[b] = nullptr;
        s.d_l[b] = nullptr;
        s.d_i[b] = nullptr;
    }
    (void)hipFree(s.d_image);
    s.d_image = nullptr;
    s.px = 0;
}

// The storage of (map, slot) for an image of geometry g, when its measurement is about to run.  The arena's pointers were
// computed at creation.  On demand (one map): the slot vector and the counts table grow to hold the slot, live counts
// moving to the new table, and the slot's buffers are allocated at exactly the geometry's pixel count.
int set_slot_bind(sfe_mapset *ms, int map, int slot, int g)
{
    sfe_ctx *ctx = ms->ctx;
    if (int rc = set_slot_check(ms, map, slot, g))
        return rc;
    if (ms->arena)
        return 0;
    if (slot >= ms->max_kf) {
        if (slot >= ms->counts_cap) {
            const int cap = 2 * (slot + 1) + 64;
            int32_t *d = nullptr;
            SFE_HIP(ctx, hipMalloc((void **)&d, sizeof(int32_t) * 2 * cap));
            SFE_HIP(ctx, hipMemsetAsync(d, 0, sizeof(int32_t) * 2 * cap, ctx->stream));
            if (ms->d_counts) {
                SFE_HIP(ctx, hipMemcpyAsync(d, ms->d_counts, sizeof(int32_t) * 2 * ms->counts_cap, hipMemcpyDeviceToDevice,
                                            ctx->stream));
                SFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
                (void)hipFree(ms->d_counts);
            }
            ms->d_counts = d;
            ms->counts_cap = cap;
        }
        ms->slots.resize(slot + 1);
        ms->max_kf = slot + 1;
        for (size_t i = 0; i < ms->slots.size(); ++i)
            ms->slots[i].d_n = ms->d_counts + 2 * i;
    }
    SetSlot &s = ms->slots[set_idx(ms, map, slot)]; // (one map: set_create)
    const int px = ms->geoms[g].img_rows * ms->geoms[g].img_cols;
    if (s.px == px)
        return 0;
    if (s.d_logodds) { // (what a measurement that failed left behind)
        (void)hipStreamSynchronize(ctx->stream);
        set_slot_free(s);
    }
    SFE_HIP(ctx, hipMalloc((void **)&s.d_logodds, px * sizeof(float)));
    for (int b = 0; b < 2; ++b) {
        SFE_HIP(ctx, hipMalloc((void **)&s.d_r[b], px * sizeof(uint16_t)));
        SFE_HIP(ctx, hipMalloc((void **)&s.d_c[b], px * sizeof(uint16_t)));
        SFE_HIP(ctx, hipMalloc((void **)&s.d_l[b], px * sizeof(float)));
        if (ms->intensity)
            SFE_HIP(ctx, hipMalloc((void **)&s.d_i[b], (size_t)px));
    }
    if (ms->intensity)
        SFE_HIP(ctx, hipMalloc((void **)&s.d_image, (size_t)px));
    s.px = px;
    return 0;
}

// pose4 per keyframe: {cos, sin, x, y}; origin2: {y0, x0}
int set_fit_jobs(sfe_mapset *ms, int n, const int32_t *maps, const int32_t *slots, const double *pose4, const double *origin2,
                 std::vector<FitJob> &jobs, int &max_px)
{
    jobs.assign(n, FitJob());
    max_px = 0;
    for (int b = 0; b < n; ++b) {
        if (int rc = set_slot_used(ms, maps[b], slots[b]))
            return rc;
        const SetSlot &s = ms->slots[set_idx(ms, maps[b], slots[b])];
        const MapGeom &g = ms->geoms[s.geom];
        FitJob &j = jobs[b];
        j.xy = g.d_xy;
        j.n_px = g.img_rows * g.img_cols;
        j.c = pose4[4 * b], j.s = pose4[4 * b + 1], j.tx = pose4[4 * b + 2], j.ty = pose4[4 * b + 3];
        j.y0 = origin2[2 * b], j.x0 = origin2[2 * b + 1];
        j.logodds = s.d_logodds;
        j.image = nullptr, j.out_i = nullptr;
        if (ms->intensity) {
            SFE_ARG(ms->ctx, s.has_image); // (sfe_mapset_set_intensity first)
            j.image = s.d_image;
        }
        max_px = max(max_px, j.n_px);
    }
    return 0;
}

// rounds of applies: round i holds the i-th apply of every map that has one
std::vector<ApplyJob> set_flat_rounds(const std::vector<std::vector<ApplyJob>> &rounds)
{
    std::vector<ApplyJob> flat;
    for (const auto &r : rounds)
        flat.insert(flat.end(), r.begin(), r.end());
    return flat;
}

// ... a launch per round; d: the rounds' jobs back to back on the device
int set_launch_rounds(sfe_mapset *ms, const ApplyJob *d, const std::vector<std::vector<ApplyJob>> &rounds)
{
    sfe_ctx *ctx = ms->ctx;
    size_t off = 0;
    for (const auto &r : rounds) {
        int px = 1;
        for (const auto &j : r)
            px = max(px, j.n_px);
        hipLaunchKernelGGL(mapset_apply_kernel, dim3((unsigned)((px + MAP_THREADS - 1) / MAP_THREADS), (unsigned)r.size()),
                           dim3(MAP_THREADS), 0, ctx->stream, d + off);
        SFE_LAUNCH_CHECK(ctx);
        ++ms->apply_launches;
        off += r.size();
    }
    return 0;
}

// the jobs' slots get their storage (before any upload from pageable memory is in flight)
int set_bind_jobs(sfe_mapset *ms, std::vector<MeasJob> &jobs, const int32_t *maps, const int32_t *slots, const int32_t *geoms)
{
    for (size_t b = 0; b < jobs.size(); ++b) {
        if (int rc = set_slot_bind(ms, maps[b], slots[b], geoms[b]))
            return rc;
        jobs[b].logodds = ms->slots[set_idx(ms, maps[b], slots[b])].d_logodds;
    }
    return 0;
}

// the measurement of a call's jobs from its hits on the device (one pair per entry; a pair outside the image leaves no
// hit): mask, filter, columns; one synchronisation; then the slots take their geometries
int set_measure_run(sfe_mapset *ms, const std::vector<MeasJob> &jobs, const int32_t *maps, const int32_t *slots,
                    const int32_t *geoms, const int32_t *d_hits, const float *ktab, int n_ktab, float miss32, float logit_miss,
                    float hit32, float logit_hit)
{
    sfe_ctx *ctx = ms->ctx;
    const int n = (int)jobs.size();
    int64_t px = 0;
    int max_px = 0, max_cols = 0;
    for (const MeasJob &j : jobs) {
        px += j.slot_px;
        max_px = max(max_px, j.slot_px);
        max_cols = max(max_cols, j.img_cols);
    }
    MeasJob *d_jobs = buf_upload(ctx, ms->buf[0], jobs.data(), jobs.size());
    float *d_k = buf_upload(ctx, ms->buf[2], ktab, (size_t)n_ktab);
    uint8_t *d_mask = (uint8_t *)buf_get(ctx, ms->buf[3], (size_t)px);
    float *d_prob = (float *)buf_get(ctx, ms->buf[4], sizeof(float) * (size_t)px);
    int32_t *d_fh = (int32_t *)buf_get(ctx, ms->buf[5], sizeof(int32_t) * (size_t)n * max_cols);
    if (!d_jobs || !d_hits || !d_k || !d_mask || !d_prob || !d_fh)
        return sfe_set_err(ctx, SFE_ERR_HIP, "map measurement scratch allocation / upload failed");
    SFE_HIP(ctx, hipMemsetAsync(d_mask, 0, (size_t)px, ctx->stream));
    const unsigned ny = (unsigned)n;
    hipLaunchKernelGGL(map_hits_kernel, dim3(4, ny), dim3(MAP_THREADS), 0, ctx->stream, d_jobs, d_hits, d_mask);
    SFE_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(map_filter_kernel, dim3((max_px + MAP_THREADS - 1) / MAP_THREADS, ny), dim3(MAP_THREADS), 0,
                       ctx->stream, d_jobs, d_k, d_mask, d_prob, hit32);
    SFE_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(map_columns_kernel, dim3((max_cols + 63) / 64, ny), dim3(64), 0, ctx->stream, d_jobs, d_prob, d_fh,
                       miss32, logit_miss, hit32, logit_hit, (int64_t)max_cols);
    SFE_LAUNCH_CHECK(ctx);
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the uploads above read pageable memory
    ms->last_meas = jobs;
    ms->last_meas_n = max_cols;
    for (int b = 0; b < n; ++b)
        ms->slots[set_idx(ms, maps[b], slots[b])].geom = geoms[b];
    return 0;
}

// the undecided points of the pending call, by ascending entry in the hit buffer
int feed_undecided(sfe_mapset *ms, float *xy_out, int32_t *pos_out, int cap)
{
    sfe_ctx *ctx = ms->ctx;
    FeedState &f = ms->feed;
    SFE_ARG(ctx, f.pending && xy_out && pos_out && cap >= f.tot_und);
    std::vector<UndPoint> und((size_t)f.tot_und);
    size_t at = 0;
    for (size_t b = 0; b < f.jobs.size(); ++b) {
        if (!f.n_und[b])
            continue;
        SFE_HIP(ctx, hipMemcpyAsync(und.data() + at, (const UndPoint *)ms->buf[9].p + f.jobs[b].hit_off,
                                    sizeof(UndPoint) * (size_t)f.n_und[b], hipMemcpyDeviceToHost, ctx->stream));
        at += (size_t)f.n_und[b];
    }
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // (the device appended them in no fixed order)
    std::sort(und.begin(), und.end(), [](const UndPoint &a, const UndPoint &b) { return a.pos < b.pos; });
    for (size_t i = 0; i < und.size(); ++i) {
        xy_out[2 * i] = und[i].x, xy_out[2 * i + 1] = und[i].y;
        pos_out[i] = und[i].pos;
    }
    return 0;
}

// the host's cells of the pending call's undecided points into the hit buffer
int feed_fill(sfe_mapset *ms, int n_cells, const int32_t *pos, const int32_t *cells)
{
    sfe_ctx *ctx = ms->ctx;
    FeedState &f = ms->feed;
    SFE_ARG(ctx, f.pending && n_cells == f.tot_und && pos && cells);
    for (int i = 0; i < n_cells; ++i)
        SFE_ARG(ctx, pos[i] >= 0 && pos[i] < f.tot);
    // (the keep flags have been read: their buffer takes the upload)
    std::vector<int32_t> up(3 * (size_t)n_cells);
    memcpy(up.data(), pos, sizeof(int32_t) * (size_t)n_cells);
    memcpy(up.data() + n_cells, cells, sizeof(int32_t) * 2 * (size_t)n_cells);
    int32_t *d_up = buf_stage(ctx, ms->buf[8], up);
    if (!d_up)
        return sfe_set_err(ctx, SFE_ERR_HIP, "map store feed: upload of the host's cells failed");
    hipLaunchKernelGGL(feed_fill_kernel, dim3((unsigned)((n_cells + 255) / 256)), dim3(256), 0, ctx->stream, d_up,
                       d_up + n_cells, n_cells, (int32_t *)ms->buf[7].p);
    SFE_LAUNCH_CHECK(ctx);
    return 0;
}

// the second half of a store-fed measurement: every entry of the hit buffer is final.  Only now do the call's slots get their
// storage, so a refused or dropped call leaves none behind.
int feed_finish(sfe_mapset *ms)
{
    FeedState &f = ms->feed;
    f.pending = false;
    if (int rc = set_bind_jobs(ms, f.jobs, f.maps.data(), f.slots.data(), f.geoms.data()))
        return rc;
    return set_measure_run(ms, f.jobs, f.maps.data(), f.slots.data(), f.geoms.data(), (const int32_t *)ms->buf[7].p,
                           f.ktab.data(), (int)f.ktab.size(), f.miss32, f.logit_miss, f.hit32, f.logit_hit);
}

// a set of n_maps zero grids; max_keyframes > 0: slots in an arena of that many per map, max_px pixels each; 0: on demand
int set_create(sfe_ctx *ctx, int n_maps, int rows, int cols, int max_keyframes, int max_px, sfe_mapset **out)
{
    SFE_ARG(ctx, out != nullptr && n_maps > 0 && n_maps <= 4096 && rows > 0 && cols > 0 && (long long)rows * cols < (1LL << 31));
    SFE_ARG(ctx, (long long)n_maps * max_keyframes < (1LL << 28));
    SFE_ARG(ctx, max_keyframes > 0 || n_maps == 1); // on demand the slot vector grows, so it is one map's
    sfe_mapset *ms = new sfe_mapset();
    ms->ctx = ctx;
    ms->arena = max_keyframes > 0;
    ms->n_maps = n_maps, ms->max_kf = max_keyframes, ms->max_px = max_px;
    ms->maps.resize(n_maps);
    const size_t n_slots = (size_t)n_maps * max_keyframes, px = n_slots * (size_t)max_px;
    ms->slots.resize(n_slots);
    int rc = 0;
    if (ms->arena) {
        bool ok = hipMalloc((void **)&ms->d_logodds, px * sizeof(float)) == hipSuccess &&
                  hipMalloc((void **)&ms->d_l, 2 * px * sizeof(float)) == hipSuccess &&
                  hipMalloc((void **)&ms->d_r, 2 * px * sizeof(uint16_t)) == hipSuccess &&
                  hipMalloc((void **)&ms->d_c, 2 * px * sizeof(uint16_t)) == hipSuccess &&
                  hipMalloc((void **)&ms->d_counts, 2 * n_slots * sizeof(int32_t)) == hipSuccess &&
                  hipMemsetAsync(ms->d_counts, 0, 2 * n_slots * sizeof(int32_t), ctx->stream) == hipSuccess;
        if (!ok)
            rc = sfe_set_err(ctx, SFE_ERR_HIP, "map set: arena of %d maps x %d keyframes x %d pixels (%zu bytes) failed", n_maps,
                             max_keyframes, max_px, px * 20);
        ms->counts_cap = (int)n_slots;
        for (size_t i = 0; i < n_slots && !rc; ++i) {
            SetSlot &s = ms->slots[i];
            s.px = max_px;
            s.d_logodds = ms->d_logodds + i * max_px;
            for (int b = 0; b < 2; ++b) {
                s.d_r[b] = ms->d_r + (2 * i + b) * max_px;
                s.d_c[b] = ms->d_c + (2 * i + b) * max_px;
                s.d_l[b] = ms->d_l + (2 * i + b) * max_px;
            }
            s.d_n = ms->d_counts + 2 * i;
        }
    }
    for (int m = 0; m < n_maps && !rc; ++m) {
        ms->maps[m].rows = rows, ms->maps[m].cols = cols;
        rc = set_grid_alloc(ms, &ms->maps[m].d_grid, (size_t)rows * cols);
    }
    if (rc) {
        sfe_mapset_destroy(ms);
        return rc;
    }
    *out = ms;
    return 0;
}

// an sfe_map is a set of one map: its handle, and the `maps` argument of a call over n of its slots
sfe_mapset *one(sfe_map *m) { return reinterpret_cast<sfe_mapset *>(m); }
std::vector<int32_t> map0(int n) { return std::vector<int32_t>(n > 0 ? n : 0, 0); }

} // namespace

extern "C" {

int sfe_mapset_create(sfe_ctx *ctx, int n_maps, int rows, int cols, int max_keyframes, int max_px, sfe_mapset **out)
{
    if (int rc = sfe_use(ctx))
        return rc;
    SFE_ARG(ctx, max_keyframes > 0 && max_px > 0 && max_px < (1 << 30));
    return set_create(ctx, n_maps, rows, cols, max_keyframes, max_px, out);
}

void sfe_mapset_destroy(sfe_mapset *ms)
{
    if (!ms)
        return;
    if (sfe_use(ms->ctx) == 0)
        (void)hipStreamSynchronize(ms->ctx->stream);
    for (auto &m : ms->maps) {
        (void)hipFree(m.d_grid);
        (void)hipFree(m.d_frames);
        (void)hipFree(m.d_inten);
        (void)hipFree(m.d_count);
    }
    for (auto &g : ms->geoms)
        (void)hipFree(g.d_xy);
    for (auto &s : ms->slots)
        if (!ms->arena)
            set_slot_free(s);
    (void)hipFree(ms->d_logodds);
    (void)hipFree(ms->d_l);
    (void)hipFree(ms->d_r);
    (void)hipFree(ms->d_c);
    (void)hipFree(ms->d_image);
    (void)hipFree(ms->d_i);
    (void)hipFree(ms->d_counts);
    for (auto &b : ms->buf)
        (void)hipFree(b.p);
    for (auto &t : ms->hit_tabs)
        (void)hipFree((void *)t.breaks); // (breaks and coef are one block)
    delete ms;
}

int sfe_mapset_geometry(sfe_mapset *ms, const float *sonar_xy, int img_rows, int img_cols, int *id_out)
{
    if (!ms)
        return SFE_ERR_ARG;
    sfe_ctx *ctx = ms->ctx;
    if (int rc = sfe_use(ctx))
        return rc;
    SFE_ARG(ctx, sonar_xy && id_out && img_rows > 0 && img_cols > 0 && (long long)img_rows * img_cols < (1 << 30));
    if (ms->arena && (long long)img_rows * img_cols > ms->max_px)
        return sfe_set_err(ctx, SFE_ERR_CAP, "map set: a %d x %d image, room for %d pixels per keyframe", img_rows, img_cols,
                           ms->max_px);
    MapGeom g;
    g.img_rows = img_rows, g.img_cols = img_cols;
    const size_t n = (size_t)img_rows * img_cols;
    SFE_HIP(ctx, hipMalloc((void **)&g.d_xy, n * sizeof(float2)));
    SFE_HIP(ctx, hipMemcpy(g.d_xy, sonar_xy, n * sizeof(float2), hipMemcpyHostToDevice));
    ms->geoms.push_back(g);
    *id_out = (int)ms->geoms.size() - 1;
    return 0;
}

int sfe_mapset_set_logodds(sfe_mapset *ms, int n, const int32_t *maps, const int32_t *slots, const int32_t *geoms,
                           const float *logodds)
{
    if (!ms)
        return SFE_ERR_ARG;
    sfe_ctx *ctx = ms->ctx;
    if (int rc = sfe_use(ctx))
        return rc;
    SFE_ARG(ctx, n >= 0 && (n == 0 || (maps && slots && geoms && logodds)));
    for (int b = 0; b < n; ++b)
        if (int rc = set_slot_check(ms, maps[b], slots[b], geoms[b]))
            return rc;
    size_t off = 0;
    for (int b = 0; b < n; ++b) {
        if (int rc = set_slot_bind(ms, maps[b], slots[b], geoms[b]))
            return rc;
        const MapGeom &g = ms->geoms[geoms[b]];
        const size_t px = (size_t)g.img_rows * g.img_cols;
        SetSlot &s = ms->slots[set_idx(ms, maps[b], slots[b])];
        SFE_HIP(ctx, hipMemcpyAsync(s.d_logodds, logodds + off, sizeof(float) * px, hipMemcpyHostToDevice, ctx->stream));
        s.geom = geoms[b];
        off += px;
    }
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int sfe_mapset_measure(sfe_mapset *ms, int n, const int32_t *maps, const int32_t *slots, const int32_t *geoms,
                       const int32_t *hit_off, const int32_t *hits, const int32_t *hrhc, const int32_t *k_off,
                       const float *ktab, int n_ktab, const double *div, float miss32, float logit_miss, float hit32,
                       float logit_hit)
{
    if (!ms)
        return SFE_ERR_ARG;
    sfe_ctx *ctx = ms->ctx;
    if (int rc = sfe_use(ctx))
        return rc;
    SFE_ARG(ctx, n >= 0 && (n == 0 || (maps && slots && geoms && hit_off && hrhc && k_off && div)) && n_ktab >= 0);
    if (n == 0)
        return 0;
    ms->feed.pending = false;
    std::vector<MeasJob> jobs(n);
    int64_t px = 0;
    for (int b = 0; b < n; ++b) {
        if (int rc = set_slot_check(ms, maps[b], slots[b], geoms[b]))
            return rc;
        const MapGeom &g = ms->geoms[geoms[b]];
        MeasJob &j = jobs[b];
        j.img_rows = g.img_rows, j.img_cols = g.img_cols, j.slot_px = g.img_rows * g.img_cols;
        j.hit_off = hit_off[b];
        j.n_hits = hit_off[b + 1] - hit_off[b];
        j.hr = hrhc[2 * b], j.hc = hrhc[2 * b + 1];
        j.k_off = k_off[b];
        // hr < 0: no points at all, the image is all miss_prob (mapping.py:224-225)
        SFE_ARG(ctx, j.n_hits >= 0 && j.hr < 1024 && j.hc < 1024 && (j.hr < 0 || j.hc >= 0));
        if (j.hr < 0)
            SFE_ARG(ctx, j.n_hits == 0);
        else
            SFE_ARG(ctx, j.k_off >= 0 && (int64_t)j.k_off + (2 * j.hr + 1) * (2 * j.hc + 1) <= n_ktab);
        j.div = div[b];
        j.px_off = px;
        px += j.slot_px;
    }
    const int n_hit_tot = hit_off[n] - hit_off[0] + 1;
    SFE_ARG(ctx, hit_off[0] == 0 && n_hit_tot >= 1 && (n_hit_tot <= 1 || hits) && (n_ktab == 0 || ktab));
    if (int rc = set_bind_jobs(ms, jobs, maps, slots, geoms))
        return rc;
    int32_t *d_hits = buf_upload(ctx, ms->buf[1], hits, 2 * (size_t)(n_hit_tot - 1));
    return set_measure_run(ms, jobs, maps, slots, geoms, d_hits, ktab, n_ktab, miss32, logit_miss, hit32, logit_hit);
}

int sfe_mapset_measure_stages(sfe_mapset *ms, int b, uint8_t *hits_out, float *prob_out, int32_t *first_hits_out)
{
    if (!ms)
        return SFE_ERR_ARG;
    sfe_ctx *ctx = ms->ctx;
    if (int rc = sfe_use(ctx))
        return rc;
    SFE_ARG(ctx, b >= 0 && b < (int)ms->last_meas.size());
    const MeasJob &j = ms->last_meas[b];
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (hits_out)
        SFE_HIP(ctx, hipMemcpy(hits_out, (uint8_t *)ms->buf[3].p + j.px_off, (size_t)j.slot_px, hipMemcpyDeviceToHost));
    if (prob_out)
        SFE_HIP(ctx, hipMemcpy(prob_out, (float *)ms->buf[4].p + j.px_off, sizeof(float) * j.slot_px, hipMemcpyDeviceToHost));
    if (first_hits_out)
        SFE_HIP(ctx, hipMemcpy(first_hits_out, (int32_t *)ms->buf[5].p + (int64_t)b * ms->last_meas_n,
                               sizeof(int32_t) * j.img_cols, hipMemcpyDeviceToHost));
    return 0;
}

int sfe_mapset_fit_bounds(sfe_mapset *ms, int n, const int32_t *maps, const int32_t *slots, const double *pose4,
                          const double *origin2, double resolution, int32_t *mm_out)
{
    if (!ms)
        return SFE_ERR_ARG;
    sfe_ctx *ctx = ms->ctx;
    if (int rc = sfe_use(ctx))
        return rc;
    SFE_ARG(ctx, n >= 0 && (n == 0 || (maps && slots && pose4 && origin2 && mm_out)) && resolution > 0);
    if (n == 0)
        return 0;
    SFE_ARG(ctx, n <= 65535);
    std::vector<FitJob> jobs;
    int max_px;
    if (int rc = set_fit_jobs(ms, n, maps, slots, pose4, origin2, jobs, max_px))
        return rc;
    std::vector<int32_t> mm(4 * (size_t)n);
    for (int b = 0; b < n; ++b)
        mm[4 * b] = INT_MAX, mm[4 * b + 1] = INT_MIN, mm[4 * b + 2] = INT_MAX, mm[4 * b + 3] = INT_MIN;
    FitJob *d_jobs = buf_upload(ctx, ms->buf[0], jobs.data(), jobs.size());
    int32_t *d_mm = buf_upload(ctx, ms->buf[1], mm.data(), mm.size());
    if (!d_jobs || !d_mm)
        return sfe_set_err(ctx, SFE_ERR_HIP, "map set fit scratch allocation / upload failed");
    const unsigned gx = (unsigned)min((max_px + MAP_THREADS - 1) / MAP_THREADS, 64);
    hipLaunchKernelGGL(map_bounds_kernel, dim3(gx, (unsigned)n), dim3(MAP_THREADS), 0, ctx->stream, d_jobs, resolution,
                       d_mm);
    SFE_LAUNCH_CHECK(ctx);
    SFE_HIP(ctx, hipMemcpyAsync(mm_out, d_mm, sizeof(int32_t) * 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int sfe_mapset_grow(sfe_mapset *ms, int n, const int32_t *maps, const int32_t *grow4)
{
    if (!ms)
        return SFE_ERR_ARG;
    sfe_ctx *ctx = ms->ctx;
    if (int rc = sfe_use(ctx))
        return rc;
    SFE_ARG(ctx, n >= 0 && (n == 0 || (maps && grow4)));
    for (int b = 0; b < n; ++b) {
        const int32_t *g = grow4 + 4 * b;
        SFE_ARG(ctx, maps[b] >= 0 && maps[b] < ms->n_maps && g[0] >= 0 && g[1] >= 0 && g[2] >= 0 && g[3] >= 0);
        for (int a = 0; a < b; ++a)
            SFE_ARG(ctx, maps[a] != maps[b]);
        const SetMap &m = ms->maps[maps[b]];
        const long long nr = (long long)m.rows + g[0] + g[1], nc = (long long)m.cols + g[2] + g[3];
        SFE_ARG(ctx, nr * nc < (1LL << 31) && nr <= 65536 && nc <= 65536);
    }
    std::vector<void *> old;
    for (int b = 0; b < n; ++b) {
        const int32_t *g = grow4 + 4 * b;
        if (g[0] + g[1] + g[2] + g[3] == 0)
            continue;
        SetMap &m = ms->maps[maps[b]];
        const int nr = m.rows + g[0] + g[1], nc = m.cols + g[2] + g[3];
        float *d = nullptr;
        uint32_t *di = nullptr;
        uint16_t *dn = nullptr;
        if (int rc = set_grid_alloc(ms, &d, (size_t)nr * nc))
            return rc;
        if (ms->intensity)
            if (int rc = set_mosaic_alloc(ms, &di, &dn, (size_t)nr * nc)) {
                (void)hipFree(d);
                return rc;
            }
        const int64_t cells = (int64_t)m.rows * m.cols;
        const dim3 pad_grid((unsigned)((cells + MAP_THREADS - 1) / MAP_THREADS));
        hipLaunchKernelGGL(map_pad_kernel<float>, pad_grid, dim3(MAP_THREADS), 0, ctx->stream, (const float *)m.d_grid, m.rows,
                           m.cols, d, nc, g[0], g[2]);
        SFE_LAUNCH_CHECK(ctx);
        old.push_back(m.d_grid);
        m.d_grid = d;
        if (ms->intensity) {
            // (on the left and right the reference raises: mapping.py:555-562, 574-581 pad columns with np.r_)
            hipLaunchKernelGGL(map_pad_kernel<uint32_t>, pad_grid, dim3(MAP_THREADS), 0, ctx->stream,
                               (const uint32_t *)m.d_inten, m.rows, m.cols, di, nc, g[0], g[2]);
            SFE_LAUNCH_CHECK(ctx);
            hipLaunchKernelGGL(map_pad_kernel<uint16_t>, pad_grid, dim3(MAP_THREADS), 0, ctx->stream,
                               (const uint16_t *)m.d_count, m.rows, m.cols, dn, nc, g[0], g[2]);
            SFE_LAUNCH_CHECK(ctx);
            old.push_back(m.d_inten);
            old.push_back(m.d_count);
            m.d_inten = di, m.d_count = dn;
        }
        m.rows = nr, m.cols = nc;
        m.grow_r += g[0], m.grow_c += g[2];
    }
    if (!old.empty()) {
        SFE_HIP(ctx, hipStreamSynchronize(ctx->stream)); // one for all the maps that grew
        for (void *p : old)
            (void)hipFree(p);
    }
    return 0;
}

int sfe_mapset_refit(sfe_mapset *ms, int n, const int32_t *maps, const int32_t *slots, const double *pose4,
                     const double *origin2, double resolution, const int32_t *mm, const int32_t *shift2, const uint8_t *dec)
{
    if (!ms)
        return SFE_ERR_ARG;
    sfe_ctx *ctx = ms->ctx;
    if (int rc = sfe_use(ctx))
        return rc;
    SFE_ARG(ctx, n >= 0 && (n == 0 || (maps && slots && pose4 && origin2 && mm && shift2 && dec)) && resolution > 0);
    if (n == 0)
        return 0;
    SFE_ARG(ctx, n <= 65535);
    std::vector<FitJob> jobs;
    int max_px;
    if (int rc = set_fit_jobs(ms, n, maps, slots, pose4, origin2, jobs, max_px))
        return rc;
    int64_t win = 0;
    std::vector<uint8_t> seen(ms->slots.size(), 0);
    for (int b = 0; b < n; ++b) {
        FitJob &j = jobs[b];
        const size_t idx = set_idx(ms, maps[b], slots[b]);
        const SetSlot &s = ms->slots[idx];
        const SetMap &m = ms->maps[maps[b]];
        SFE_ARG(ctx, !seen[idx]); // one refit per slot and call: its other buffer takes the new list
        seen[idx] = 1;
        SFE_ARG(ctx, mm[4 * b] <= mm[4 * b + 1] && mm[4 * b + 2] <= mm[4 * b + 3]);
        j.wr0 = mm[4 * b], j.wh = mm[4 * b + 1] - mm[4 * b] + 1;
        j.wc0 = mm[4 * b + 2], j.ww = mm[4 * b + 3] - mm[4 * b + 2] + 1;
        j.sr = shift2[2 * b], j.sc = shift2[2 * b + 1];
        // every cell inside its map's grid as it stands now (the caller grew it first)
        SFE_ARG(ctx, j.wr0 + j.sr >= 0 && j.wr0 + j.sr + j.wh <= m.rows && j.wc0 + j.sc >= 0 && j.wc0 + j.sc + j.ww <= m.cols);
        SFE_ARG(ctx, (int64_t)j.wh * j.ww < (1LL << 30));
        SFE_ARG(ctx, !dec[b] || s.has_cells);
        j.win_off = win; // each keyframe's own window, back to back: the largest map sizes nothing
        win += (int64_t)j.wh * j.ww;
        const int nb = 1 - s.cur;
        j.out_r = s.d_r[nb], j.out_c = s.d_c[nb], j.out_l = s.d_l[nb];
        j.out_n = s.d_n + nb;
        j.out_i = ms->intensity ? s.d_i[nb] : nullptr;
    }
    SFE_ARG(ctx, win < (1LL << 40));
    // room for both job tables (the fits, then up to two applies per fit) and the windows, before any state changes
    static_assert(sizeof(FitJob) % alignof(ApplyJob) == 0, "the apply jobs follow the fit jobs in one table");
    const size_t fit_bytes = sizeof(FitJob) * (size_t)n;
    int32_t *d_win = (int32_t *)buf_get(ctx, ms->buf[1], sizeof(int32_t) * (size_t)win);
    if (!buf_get(ctx, ms->buf[0], fit_bytes + 2 * sizeof(ApplyJob) * (size_t)n) || !d_win)
        return sfe_set_err(ctx, SFE_ERR_HIP, "map set fit scratch allocation failed");
    // the float32 history of every cell as the reference writes it, per map: for each of its keyframes in call order, dec
    // then inc.  Maps do not share cells, so the i-th apply of every map goes into round i.
    std::vector<std::vector<ApplyJob>> rounds;
    std::vector<int> seq(ms->n_maps, 0);
    for (int b = 0; b < n; ++b) {
        SetSlot &s = ms->slots[set_idx(ms, maps[b], slots[b])];
        SetMap &m = ms->maps[maps[b]];
        ApplyJob a;
        a.grid = m.d_grid, a.rows = m.rows, a.cols = m.cols, a.n_px = jobs[b].n_px;
        a.grid_i = m.d_inten, a.grid_n = m.d_count; // (null unless the mosaic is enabled)
        for (int pass = dec[b] ? 0 : 1; pass < 2; ++pass) {
            const int o = pass ? 1 - s.cur : s.cur;
            a.r = s.d_r[o], a.c = s.d_c[o], a.l = s.d_l[o];
            a.i = s.d_i[o];
            a.n = s.d_n + o;
            a.dr = pass ? 0 : m.grow_r - s.base_r, a.dc = pass ? 0 : m.grow_c - s.base_c;
            a.sub = pass ? 0 : 1;
            const int round = seq[maps[b]]++;
            if (round >= (int)rounds.size())
                rounds.resize(round + 1);
            rounds[round].push_back(a);
        }
        s.cur = 1 - s.cur;
        s.has_cells = 1;
        s.base_r = m.grow_r, s.base_c = m.grow_c;
    }
    // both job tables in one upload through pinned staging: the call only enqueues (no synchronisation per batch)
    const std::vector<ApplyJob> flat = set_flat_rounds(rounds);
    std::vector<char> tab(fit_bytes + sizeof(ApplyJob) * flat.size());
    memcpy(tab.data(), jobs.data(), fit_bytes);
    memcpy(tab.data() + fit_bytes, flat.data(), sizeof(ApplyJob) * flat.size());
    char *d_tab = buf_stage(ctx, ms->buf[0], tab);
    if (!d_tab)
        return sfe_set_err(ctx, SFE_ERR_HIP, "map set: fit / apply job table upload failed");
    const FitJob *d_jobs = (const FitJob *)d_tab;
    SFE_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)d_win, EMPTY_SLOT, (size_t)win, ctx->stream));
    hipLaunchKernelGGL(map_scatter_kernel, dim3((unsigned)((max_px + MAP_THREADS - 1) / MAP_THREADS), (unsigned)n),
                       dim3(MAP_THREADS), 0, ctx->stream, d_jobs, resolution, d_win);
    SFE_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(map_compact_kernel, dim3((unsigned)n), dim3(COMPACT_THREADS), 0, ctx->stream, d_jobs, d_win);
    SFE_LAUNCH_CHECK(ctx);
    return set_launch_rounds(ms, (const ApplyJob *)(d_tab + fit_bytes), rounds);
}

int sfe_mapset_cells(sfe_mapset *ms, int map, int slot, uint16_t *r_out, uint16_t *c_out, float *l_out, int cap, int *n_out)
{
    if (!ms)
        return SFE_ERR_ARG;
    sfe_ctx *ctx = ms->ctx;
    if (int rc = sfe_use(ctx))
        return rc;
    if (int rc = set_slot_used(ms, map, slot))
        return rc;
    const SetSlot &s = ms->slots[set_idx(ms, map, slot)];
    const SetMap &m = ms->maps[map];
    SFE_ARG(ctx, s.has_cells && n_out);
    int32_t n = 0;
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    SFE_HIP(ctx, hipMemcpy(&n, s.d_n + s.cur, sizeof(int32_t), hipMemcpyDeviceToHost));
    *n_out = n;
    if (n > cap)
        return sfe_set_err(ctx, SFE_ERR_CAP, "map set cells: %d cells, room for %d", n, cap);
    if (r_out)
        SFE_HIP(ctx, hipMemcpy(r_out, s.d_r[s.cur], sizeof(uint16_t) * n, hipMemcpyDeviceToHost));
    if (c_out)
        SFE_HIP(ctx, hipMemcpy(c_out, s.d_c[s.cur], sizeof(uint16_t) * n, hipMemcpyDeviceToHost));
    if (l_out)
        SFE_HIP(ctx, hipMemcpy(l_out, s.d_l[s.cur], sizeof(float) * n, hipMemcpyDeviceToHost));
    // the growth since the list was written (uint16 arithmetic, as the reference's keyframe.r += inc_r)
    for (int i = 0; r_out && i < n; ++i)
        r_out[i] = (uint16_t)(r_out[i] + (m.grow_r - s.base_r));
    for (int i = 0; c_out && i < n; ++i)
        c_out[i] = (uint16_t)(c_out[i] + (m.grow_c - s.base_c));
    return 0;
}

int sfe_mapset_logodds(sfe_mapset *ms, int map, int slot, float *out, int cap)
{
    if (!ms)
        return SFE_ERR_ARG;
    sfe_ctx *ctx = ms->ctx;
    if (int rc = sfe_use(ctx))
        return rc;
    if (int rc = set_slot_used(ms, map, slot))
        return rc;
    const SetSlot &s = ms->slots[set_idx(ms, map, slot)];
    const MapGeom &g = ms->geoms[s.geom];
    SFE_ARG(ctx, out && cap >= g.img_rows * g.img_cols);
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    SFE_HIP(ctx, hipMemcpy(out, s.d_logodds, sizeof(float) * g.img_rows * g.img_cols, hipMemcpyDeviceToHost));
    return 0;
}

int sfe_mapset_shape(sfe_mapset *ms, int map, int32_t *rows_cols_grow4)
{
    if (!ms || !rows_cols_grow4 || map < 0 || map >= ms->n_maps)
        return SFE_ERR_ARG;
    const SetMap &m = ms->maps[map];
    rows_cols_grow4[0] = m.rows, rows_cols_grow4[1] = m.cols;
    rows_cols_grow4[2] = m.grow_r, rows_cols_grow4[3] = m.grow_c;
    return 0;
}

int sfe_mapset_apply_launches(sfe_mapset *ms, long long *n_out)
{
    if (!ms || !n_out)
        return SFE_ERR_ARG;
    *n_out = ms->apply_launches;
    return 0;
}

// which = 0: the map's grid; 1: the grid of its last sfe_mapset_frames call
int sfe_mapset_read_grid(sfe_mapset *ms, int map, int which, float *out, long long cap)
{
    if (!ms)
        return SFE_ERR_ARG;
    sfe_ctx *ctx = ms->ctx;
    if (int rc = sfe_use(ctx))
        return rc;
    SFE_ARG(ctx, map >= 0 && map < ms->n_maps);
    const SetMap &m = ms->maps[map];
    const float *src = which ? m.d_frames : m.d_grid;
    const long long n = which ? (long long)m.frames_rows * m.frames_cols : (long long)m.rows * m.cols;
    SFE_ARG(ctx, out && src && cap >= n);
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    SFE_HIP(ctx, hipMemcpy(out, src, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}

// get_occupancy_grid1(frames=...): per map a fresh zero grid, the listed slots' cells added in list order
int sfe_mapset_frames(sfe_mapset *ms, int n_maps, const int32_t *maps, const int32_t *slot_off, const int32_t *slots)
{
    if (!ms)
        return SFE_ERR_ARG;
    sfe_ctx *ctx = ms->ctx;
    if (int rc = sfe_use(ctx))
        return rc;
    SFE_ARG(ctx, n_maps >= 0 && (n_maps == 0 || (maps && slot_off)) && (n_maps == 0 || slot_off[0] == 0));
    for (int b = 0; b < n_maps; ++b) {
        SFE_ARG(ctx, maps[b] >= 0 && maps[b] < ms->n_maps && slot_off[b + 1] >= slot_off[b]);
        SFE_ARG(ctx, slot_off[b + 1] == slot_off[b] || slots);
        for (int a = 0; a < b; ++a)
            SFE_ARG(ctx, maps[a] != maps[b]);
        for (int i = slot_off[b]; i < slot_off[b + 1]; ++i) {
            if (int rc = set_slot_used(ms, maps[b], slots[i]))
                return rc;
            SFE_ARG(ctx, ms->slots[set_idx(ms, maps[b], slots[i])].has_cells);
        }
    }
    std::vector<std::vector<ApplyJob>> rounds;
    for (int b = 0; b < n_maps; ++b) {
        SetMap &m = ms->maps[maps[b]];
        if (m.frames_rows != m.rows || m.frames_cols != m.cols) {
            (void)hipStreamSynchronize(ctx->stream);
            (void)hipFree(m.d_frames);
            m.d_frames = nullptr;
            m.frames_rows = m.frames_cols = 0;
            if (int rc = set_grid_alloc(ms, &m.d_frames, (size_t)m.rows * m.cols))
                return rc;
            m.frames_rows = m.rows, m.frames_cols = m.cols;
        } else
            SFE_HIP(ctx, hipMemsetAsync(m.d_frames, 0, sizeof(float) * (size_t)m.rows * m.cols, ctx->stream));
        for (int i = slot_off[b]; i < slot_off[b + 1]; ++i) {
            const SetSlot &s = ms->slots[set_idx(ms, maps[b], slots[i])];
            const MapGeom &g = ms->geoms[s.geom];
            ApplyJob a;
            a.grid = m.d_frames, a.rows = m.rows, a.cols = m.cols, a.n_px = g.img_rows * g.img_cols;
            a.grid_i = nullptr, a.grid_n = nullptr, a.i = nullptr; // (the mosaic has no frames= form)
            a.r = s.d_r[s.cur], a.c = s.d_c[s.cur], a.l = s.d_l[s.cur];
            a.n = s.d_n + s.cur;
            a.dr = m.grow_r - s.base_r, a.dc = m.grow_c - s.base_c, a.sub = 0;
            const int round = i - slot_off[b];
            if (round >= (int)rounds.size())
                rounds.resize(round + 1);
            rounds[round].push_back(a);
        }
    }
    const std::vector<ApplyJob> flat = set_flat_rounds(rounds);
    if (flat.empty())
        return 0;
    const ApplyJob *d = buf_stage(ctx, ms->buf[2], flat);
    if (!d)
        return sfe_set_err(ctx, SFE_ERR_HIP, "map set: apply job table upload failed");
    return set_launch_rounds(ms, d, rounds);
}

int sfe_mapset_render(sfe_mapset *ms, int n, const int32_t *maps, const int32_t *which, const int32_t *box4,
                      const int32_t *out_hw, const double *inv, const int32_t *resize, const long long *out_off,
                      int8_t *occ_out, long long total)
{
    if (!ms)
        return SFE_ERR_ARG;
    sfe_ctx *ctx = ms->ctx;
    if (int rc = sfe_use(ctx))
        return rc;
    SFE_ARG(ctx, n >= 0 && total >= 0 && (n == 0 || (maps && which && box4 && out_hw && inv && resize && out_off)));
    SFE_ARG(ctx, n <= 65535 && (total == 0 || occ_out));
    std::vector<RenderJob> jobs;
    int64_t max_out = 0;
    for (int b = 0; b < n; ++b) {
        SFE_ARG(ctx, maps[b] >= 0 && maps[b] < ms->n_maps);
        const SetMap &m = ms->maps[maps[b]];
        RenderJob j;
        j.grid = which[b] ? m.d_frames : m.d_grid;
        SFE_ARG(ctx, j.grid && (!which[b] || (m.frames_rows == m.rows && m.frames_cols == m.cols)));
        const int r0 = box4[4 * b], r1 = box4[4 * b + 1], c0 = box4[4 * b + 2], c1 = box4[4 * b + 3];
        j.oh = out_hw[2 * b], j.ow = out_hw[2 * b + 1];
        SFE_ARG(ctx, j.oh >= 0 && j.ow >= 0);
        const int64_t cells = (int64_t)j.oh * j.ow;
        if (cells == 0)
            continue;
        j.cols = m.cols, j.r0 = r0, j.c0 = c0, j.h = r1 - r0 + 1, j.w = c1 - c0 + 1;
        j.resize = resize[b], j.inv = inv[b], j.out_off = out_off[b];
        SFE_ARG(ctx, r0 >= 0 && c0 >= 0 && j.h > 0 && j.w > 0 && r1 < m.rows && c1 < m.cols);
        SFE_ARG(ctx, j.resize || (j.oh == j.h && j.ow == j.w));
        SFE_ARG(ctx, !j.resize || j.inv > 0);
        SFE_ARG(ctx, j.out_off >= 0 && j.out_off + cells <= total);
        max_out = max(max_out, cells);
        jobs.push_back(j);
    }
    if (jobs.empty())
        return 0;
    RenderJob *d_jobs = buf_stage(ctx, ms->buf[0], jobs);
    int8_t *d = (int8_t *)buf_get(ctx, ms->buf[1], (size_t)total);
    if (!d_jobs || !d)
        return sfe_set_err(ctx, SFE_ERR_HIP, "map set render scratch allocation / upload failed");
    const unsigned gx = (unsigned)std::min<int64_t>((max_out + MAP_THREADS - 1) / MAP_THREADS, 1 << 20);
    hipLaunchKernelGGL(mapset_render_kernel, dim3(gx, (unsigned)jobs.size()), dim3(MAP_THREADS), 0, ctx->stream, d_jobs, d);
    SFE_LAUNCH_CHECK(ctx);
    // (bytes of `total` no job covers are whatever the scratch held: the offsets are the caller's)
    SFE_HIP(ctx, hipMemcpyAsync(occ_out, d, (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// ---- the intensity mosaic (sonarfe.h) ----------------------------------------------------------------------------------------
int sfe_mapset_enable_intensity(sfe_mapset *ms)
{
    if (!ms)
        return SFE_ERR_ARG;
    sfe_ctx *ctx = ms->ctx;
    if (int rc = sfe_use(ctx))
        return rc;
    if (ms->intensity)
        return 0;
    SFE_ARG(ctx, ms->geoms.empty()); // before the first geometry ...
    for (const SetSlot &s : ms->slots)
        SFE_ARG(ctx, s.geom < 0 && s.px == (ms->arena ? ms->max_px : 0)); // ... and the first slot
    if (ms->arena) {
        const size_t px = ms->slots.size() * (size_t)ms->max_px;
        if (hipMalloc((void **)&ms->d_image, px) != hipSuccess || hipMalloc((void **)&ms->d_i, 2 * px) != hipSuccess) {
            (void)hipFree(ms->d_image);
            ms->d_image = ms->d_i = nullptr;
            return sfe_set_err(ctx, SFE_ERR_HIP, "map set: intensity arena of %zu bytes failed", 3 * px);
        }
    }
    for (SetMap &m : ms->maps)
        if (int rc = set_mosaic_alloc(ms, &m.d_inten, &m.d_count, (size_t)m.rows * m.cols)) {
            for (SetMap &k : ms->maps) {
                (void)hipFree(k.d_inten);
                (void)hipFree(k.d_count);
                k.d_inten = nullptr, k.d_count = nullptr;
            }
            (void)hipFree(ms->d_image);
            (void)hipFree(ms->d_i);
            ms->d_image = ms->d_i = nullptr;
            return rc;
        }
    if (ms->arena)
        for (size_t i = 0; i < ms->slots.size(); ++i) {
            SetSlot &s = ms->slots[i];
            s.d_image = ms->d_image + i * ms->max_px;
            for (int b = 0; b < 2; ++b)
                s.d_i[b] = ms->d_i + (2 * i + b) * ms->max_px;
        }
    ms->intensity = true;
    return 0;
}

// The checks of an intensity upload, then (with `images`) one upload of all n full-size images through the pinned staging,
// one launch of the sampler over the jobs.  shape4[4 b ..] = {full_rows, full_cols, r_skip, c_skip}.
static int set_intensity(sfe_mapset *ms, int n, const int32_t *maps, const int32_t *slots, const int32_t *geoms,
                         const int32_t *shape4, const uint8_t *images, const void *const *d_images, const long long *stride)
{
    if (!ms)
        return SFE_ERR_ARG;
    sfe_ctx *ctx = ms->ctx;
    if (int rc = sfe_use(ctx))
        return rc;
    SFE_ARG(ctx, ms->intensity && n >= 0 && n <= 65535);
    SFE_ARG(ctx, n == 0 || (maps && slots && geoms && shape4 && (images || (d_images && stride))));
    if (n == 0)
        return 0;
    size_t total = 0;
    int max_px = 1;
    std::vector<std::pair<int32_t, int32_t>> named(n);
    for (int b = 0; b < n; ++b) {
        if (int rc = set_slot_check(ms, maps[b], slots[b], geoms[b]))
            return rc;
        named[b] = {maps[b], slots[b]};
        const MapGeom &g = ms->geoms[geoms[b]];
        const int32_t fr = shape4[4 * b], fc = shape4[4 * b + 1], rs = shape4[4 * b + 2], cs = shape4[4 * b + 3];
        SFE_ARG(ctx, fr > 0 && fc > 0 && rs >= 1 && cs >= 1 && (long long)fr * fc < (1LL << 31));
        // the full image is num_ranges x num_bearings of the slot's geometry
        if ((fr + rs - 1) / rs != g.img_rows || (fc + cs - 1) / cs != g.img_cols)
            return sfe_set_err(ctx, SFE_ERR_ARG, "map set intensity: a %d x %d image at skips %d, %d is %d x %d, the geometry's "
                               "image is %d x %d (job %d)", fr, fc, rs, cs, (fr + rs - 1) / rs, (fc + cs - 1) / cs, g.img_rows,
                               g.img_cols, b);
        if (!images) {
            // every sampled byte inside the rows the caller describes
            SFE_ARG(ctx, d_images[b] && stride[b] >= fc);
        }
        total += (size_t)fr * fc;
        max_px = max(max_px, g.img_rows * g.img_cols);
    }
    std::sort(named.begin(), named.end());
    SFE_ARG(ctx, std::adjacent_find(named.begin(), named.end()) == named.end()); // a slot holds one image
    uint8_t *d_full = nullptr;
    void *pin = nullptr;
    if (images) {
        d_full = (uint8_t *)buf_get(ctx, ms->buf[20], total);
        pin = d_full ? sfe_pinned_begin(ctx, total) : nullptr;
        if (!d_full || !pin)
            return sfe_set_err(ctx, SFE_ERR_HIP, "map set intensity: staging of %zu bytes failed", total);
    }
    std::vector<SampleJob> jobs(n);
    size_t off = 0;
    for (int b = 0; b < n; ++b) {
        if (int rc = set_slot_bind(ms, maps[b], slots[b], geoms[b]))
            return rc;
        const MapGeom &g = ms->geoms[geoms[b]];
        SetSlot &s = ms->slots[set_idx(ms, maps[b], slots[b])];
        SampleJob &j = jobs[b];
        j.img_rows = g.img_rows, j.img_cols = g.img_cols, j.r_skip = shape4[4 * b + 2], j.c_skip = shape4[4 * b + 3];
        j.out = s.d_image;
        if (images) {
            j.src = d_full + off, j.stride = shape4[4 * b + 1];
            off += (size_t)shape4[4 * b] * shape4[4 * b + 1];
        } else {
            j.src = (const uint8_t *)d_images[b], j.stride = stride[b];
        }
    }
    if (images) {
        memcpy(pin, images, total);
        SFE_HIP(ctx, hipMemcpyAsync(d_full, pin, total, hipMemcpyHostToDevice, ctx->stream));
        if (sfe_pinned_end(ctx, ctx->stream))
            return sfe_set_err(ctx, SFE_ERR_HIP, "map set intensity: staging failed");
    }
    const SampleJob *d_jobs = buf_stage(ctx, ms->buf[19], jobs);
    if (!d_jobs)
        return sfe_set_err(ctx, SFE_ERR_HIP, "map set intensity: job table upload failed");
    hipLaunchKernelGGL(map_sample_kernel, dim3((unsigned)((max_px + MAP_THREADS - 1) / MAP_THREADS), (unsigned)n),
                       dim3(MAP_THREADS), 0, ctx->stream, d_jobs);
    SFE_LAUNCH_CHECK(ctx);
    for (int b = 0; b < n; ++b) {
        SetSlot &s = ms->slots[set_idx(ms, maps[b], slots[b])];
        s.geom = geoms[b];
        s.has_image = 1;
    }
    return 0;
}

int sfe_mapset_set_intensity(sfe_mapset *ms, int n, const int32_t *maps, const int32_t *slots, const int32_t *geoms,
                             const int32_t *shape4, const uint8_t *images)
{
    if (ms && n > 0)
        SFE_ARG(ms->ctx, images);
    return set_intensity(ms, n, maps, slots, geoms, shape4, images, nullptr, nullptr);
}

int sfe_mapset_set_intensity_dev(sfe_mapset *ms, int n, const int32_t *maps, const int32_t *slots, const int32_t *geoms,
                                 const int32_t *shape4, const void *const *d_images, const long long *row_stride)
{
    if (ms && n > 0)
        SFE_ARG(ms->ctx, d_images && row_stride);
    return set_intensity(ms, n, maps, slots, geoms, shape4, nullptr, d_images, row_stride);
}

int sfe_mapset_render_intensity(sfe_mapset *ms, int n, const int32_t *maps, const int32_t *box4, const long long *out_off,
                                long long total, int8_t *out)
{
    if (!ms)
        return SFE_ERR_ARG;
    sfe_ctx *ctx = ms->ctx;
    if (int rc = sfe_use(ctx))
        return rc;
    SFE_ARG(ctx, ms->intensity && n >= 0 && n <= 65535 && total >= 0 && (total == 0 || out));
    SFE_ARG(ctx, n == 0 || (maps && box4 && out_off));
    std::vector<RenderIJob> jobs;
    int64_t max_out = 0;
    for (int b = 0; b < n; ++b) {
        SFE_ARG(ctx, maps[b] >= 0 && maps[b] < ms->n_maps);
        const SetMap &m = ms->maps[maps[b]];
        const int r0 = box4[4 * b], r1 = box4[4 * b + 1], c0 = box4[4 * b + 2], c1 = box4[4 * b + 3];
        RenderIJob j;
        j.grid_i = m.d_inten, j.grid_n = m.d_count, j.cols = m.cols;
        j.r0 = r0, j.c0 = c0, j.h = r1 - r0 + 1, j.w = c1 - c0 + 1, j.out_off = out_off[b];
        SFE_ARG(ctx, r0 >= 0 && c0 >= 0 && j.h > 0 && j.w > 0 && r1 < m.rows && c1 < m.cols);
        SFE_ARG(ctx, j.out_off >= 0 && j.out_off + (int64_t)j.h * j.w <= total);
        max_out = max(max_out, (int64_t)j.h * j.w);
        jobs.push_back(j);
    }
    if (jobs.empty())
        return 0;
    const RenderIJob *d_jobs = buf_stage(ctx, ms->buf[0], jobs);
    int8_t *d = (int8_t *)buf_get(ctx, ms->buf[1], (size_t)total);
    if (!d_jobs || !d)
        return sfe_set_err(ctx, SFE_ERR_HIP, "map set intensity render scratch allocation / upload failed");
    const unsigned gx = (unsigned)std::min<int64_t>((max_out + MAP_THREADS - 1) / MAP_THREADS, 1 << 20);
    hipLaunchKernelGGL(mapset_render_intensity_kernel, dim3(gx, (unsigned)jobs.size()), dim3(MAP_THREADS), 0, ctx->stream,
                       d_jobs, d);
    SFE_LAUNCH_CHECK(ctx);
    // (bytes of `total` no job covers are whatever the scratch held: the offsets are the caller's)
    SFE_HIP(ctx, hipMemcpyAsync(out, d, (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int sfe_mapset_read_intensity(sfe_mapset *ms, int map, uint32_t *intensity_out, uint16_t *counter_out, long long cap)
{
    if (!ms)
        return SFE_ERR_ARG;
    sfe_ctx *ctx = ms->ctx;
    if (int rc = sfe_use(ctx))
        return rc;
    SFE_ARG(ctx, ms->intensity && map >= 0 && map < ms->n_maps);
    const SetMap &m = ms->maps[map];
    const long long n = (long long)m.rows * m.cols;
    SFE_ARG(ctx, cap >= n && (intensity_out || counter_out));
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (intensity_out)
        SFE_HIP(ctx, hipMemcpy(intensity_out, m.d_inten, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost));
    if (counter_out)
        SFE_HIP(ctx, hipMemcpy(counter_out, m.d_count, sizeof(uint16_t) * (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}

int sfe_mapset_slot_intensity(sfe_mapset *ms, int map, int slot, uint8_t *image_out, int image_cap, uint8_t *i_out,
                              int cells_cap, int *n_out)
{
    if (!ms)
        return SFE_ERR_ARG;
    sfe_ctx *ctx = ms->ctx;
    if (int rc = sfe_use(ctx))
        return rc;
    SFE_ARG(ctx, ms->intensity);
    if (int rc = set_slot_used(ms, map, slot))
        return rc;
    const SetSlot &s = ms->slots[set_idx(ms, map, slot)];
    const MapGeom &g = ms->geoms[s.geom];
    SFE_ARG(ctx, s.has_image);
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (image_out) {
        SFE_ARG(ctx, image_cap >= g.img_rows * g.img_cols);
        SFE_HIP(ctx, hipMemcpy(image_out, s.d_image, (size_t)g.img_rows * g.img_cols, hipMemcpyDeviceToHost));
    }
    if (i_out || n_out) {
        // (the payload of a cell does not move with the growth that shifts its r and c: sfe_mapset_cells)
        SFE_ARG(ctx, s.has_cells);
        int32_t n = 0;
        SFE_HIP(ctx, hipMemcpy(&n, s.d_n + s.cur, sizeof(int32_t), hipMemcpyDeviceToHost));
        if (n_out)
            *n_out = n;
        if (i_out) {
            if (n > cells_cap)
                return sfe_set_err(ctx, SFE_ERR_CAP, "map set slot intensity: %d cells, room for %d", n, cells_cap);
            SFE_HIP(ctx, hipMemcpy(i_out, s.d_i[s.cur], (size_t)n, hipMemcpyDeviceToHost));
        }
    }
    return 0;
}

// get_occupancy_grid2 for n images in one call and one read-back.  Job b: map maps[b]; the free cells are the current lists of
// slots[slot_off[b] .. slot_off[b + 1]); the known region is box4[4 b ..] = {r0, r1, c0, c1} (the union of those lists' boxes:
// the caller's), its corner origin2[2 b ..] = {y0, x0} metres; its points xy[2 pt_off[b] .. 2 pt_off[b + 1]) (float64 x, y).
// Where a render2 call's points come from: the host (pt_off / xy), or clouds of a store (`store` set), taken in place.
struct Render2Src {
    const int32_t *pt_off = nullptr;
    const double *xy = nullptr;
    sfe_cloud_store *store = nullptr;
    const int32_t *handles = nullptr, *all_frames = nullptr, *frame_off = nullptr, *frames = nullptr;
};

static int set_render2(sfe_mapset *ms, const Render2Src &src, int n, const int32_t *maps, const int32_t *slot_off,
                       const int32_t *slots, const int32_t *box4, const int32_t *filter, const double *radius,
                       const int32_t *min_points, const int32_t *dilate_hs, const double *origin2, const double *resolution,
                       const int32_t *out_hw, const double *inv, const int32_t *resize, const long long *out_off,
                       int8_t *occ_out, long long total)
{
    if (!ms)
        return SFE_ERR_ARG;
    sfe_ctx *ctx = ms->ctx;
    if (int rc = sfe_use(ctx))
        return rc;
    const int32_t *pt_off = src.pt_off;
    const double *xy = src.xy;
    SFE_ARG(ctx, n >= 0 && n <= 65535 && total >= 0 && (total == 0 || occ_out));
    SFE_ARG(ctx, n == 0 || (maps && slot_off && box4 && filter && radius && min_points && dilate_hs && origin2 && resolution &&
                            out_hw && inv && resize && out_off));
    SfeStoreView v = {};
    if (src.store) {
        SFE_ARG(ctx, sfe_store_ctx(src.store) == ctx && (n == 0 || (src.handles && src.all_frames && src.frame_off)));
    } else {
        SFE_ARG(ctx, n == 0 || pt_off);
    }
    if (n == 0)
        return 0;
    SFE_ARG(ctx, slot_off[0] == 0 && (src.store ? src.frame_off[0] == 0 : pt_off[0] == 0));
    if (src.store)
        if (int rc = sfe_store_view(src.store, &v))
            return rc;
    int64_t tot_pts = 0; // the store route's point table: mult / keep entries
    std::vector<Render2Job> jobs;
    std::vector<MarkJob> marks;
    std::vector<int64_t> mark_work; // the work image of each list, as an offset until the scratch is there
    std::vector<int32_t> spans;
    std::vector<std::pair<int, int>> span_at; // (half size, offset) of the elements already in `spans`
    int64_t work = 0, max_out = 0, max_stamp = 0;
    int max_px = 1, max_pts = 0;
    bool any_filter = false;
    for (int b = 0; b < n; ++b) {
        SFE_ARG(ctx, maps[b] >= 0 && maps[b] < ms->n_maps);
        SFE_ARG(ctx, slot_off[b + 1] >= slot_off[b] && (slot_off[b + 1] == slot_off[b] || slots));
        SFE_ARG(ctx, src.store || (pt_off[b + 1] >= pt_off[b] && (pt_off[b + 1] == pt_off[b] || xy)));
        const SetMap &m = ms->maps[maps[b]];
        const int r0 = box4[4 * b], r1 = box4[4 * b + 1], c0 = box4[4 * b + 2], c1 = box4[4 * b + 3];
        Render2Job j;
        j.h = r1 - r0 + 1, j.w = c1 - c0 + 1, j.oh = out_hw[2 * b], j.ow = out_hw[2 * b + 1];
        j.resize = resize[b], j.inv = inv[b], j.out_off = out_off[b];
        SFE_ARG(ctx, r0 >= 0 && c0 >= 0 && j.h > 0 && j.w > 0 && r1 < m.rows && c1 < m.cols);
        SFE_ARG(ctx, j.oh >= 0 && j.ow >= 0 && (j.resize ? j.inv > 0 : (j.oh == j.h && j.ow == j.w)));
        SFE_ARG(ctx, j.out_off >= 0 && j.out_off + (int64_t)j.oh * j.ow <= total);
        j.pool_off = 0, j.frame_off = 0, j.n_frames = -1;
        if (src.store) {
            const int hd = src.handles[b];
            if (hd < 0 || hd >= v.n_slots || v.cnt[hd] < 0)
                return sfe_set_err(ctx, SFE_ERR_ARG, "map set render2: cloud %d named (job %d), the store holds %d%s", hd, b,
                                   v.n_slots, (hd >= 0 && hd < v.n_slots) ? " and that one was not stored" : "");
            SFE_ARG(ctx, src.frame_off[b + 1] >= src.frame_off[b] && (src.frame_off[b + 1] == src.frame_off[b] || src.frames));
            if (!src.all_frames[b]) {
                if (!v.d_key || hd >= v.n_keyed || !v.keyed[hd])
                    return sfe_set_err(ctx, SFE_ERR_ARG, "map set render2: a frame list for cloud %d (job %d), which has no keys "
                                       "(it was not built by a keyed entry point)", hd, b);
                j.frame_off = src.frame_off[b], j.n_frames = src.frame_off[b + 1] - src.frame_off[b];
            }
            j.pool_off = v.off[hd];
            j.pt_off = (int32_t)tot_pts, j.n_pts = v.cnt[hd];
            tot_pts += j.n_pts;
            SFE_ARG(ctx, tot_pts < (1 << 30));
        } else {
            j.pt_off = pt_off[b], j.n_pts = pt_off[b + 1] - pt_off[b];
        }
        j.filter = filter[b] != 0, j.min_points = min_points[b], j.r2 = (float)(radius[b] * radius[b]);
        j.hs = dilate_hs[b];
        SFE_ARG(ctx, j.hs >= 0 && j.hs <= 4096 && resolution[b] > 0);
        j.y0 = origin2[2 * b], j.x0 = origin2[2 * b + 1], j.res = resolution[b];
        j.span_off = -1;
        for (const auto &e : span_at)
            if (e.first == j.hs)
                j.span_off = e.second;
        if (j.span_off < 0) {
            j.span_off = (int)spans.size();
            span_at.push_back({j.hs, j.span_off});
            const std::vector<int32_t> sp = cost_ellipse_spans(j.hs);
            spans.insert(spans.end(), sp.begin(), sp.end());
        }
        j.work_off = work;
        work += (int64_t)j.h * j.w;
        for (int i = slot_off[b]; i < slot_off[b + 1]; ++i) {
            if (int rc = set_slot_used(ms, maps[b], slots[i]))
                return rc;
            const SetSlot &s = ms->slots[set_idx(ms, maps[b], slots[i])];
            SFE_ARG(ctx, s.has_cells);
            MarkJob k;
            k.img = nullptr, k.h = j.h, k.w = j.w;
            k.r = s.d_r[s.cur], k.c = s.d_c[s.cur], k.n = s.d_n + s.cur;
            k.dr = m.grow_r - s.base_r - r0, k.dc = m.grow_c - s.base_c - c0;
            k.n_px = ms->geoms[s.geom].img_rows * ms->geoms[s.geom].img_cols;
            max_px = max(max_px, k.n_px);
            marks.push_back(k);
            mark_work.push_back(j.work_off);
        }
        max_out = max(max_out, (int64_t)j.oh * j.ow);
        max_pts = max(max_pts, j.n_pts);
        max_stamp = max(max_stamp, (int64_t)j.n_pts * (2 * j.hs + 1));
        any_filter = any_filter || (j.filter && j.n_pts > 0);
        jobs.push_back(j);
    }
    SFE_ARG(ctx, marks.size() <= 65535 && work < (1LL << 40));
    const int n_pts = src.store ? (int)tot_pts : pt_off[n];
    const int64_t n16 = (work + 15) / 16;
    int8_t *d_work = (int8_t *)buf_get(ctx, ms->buf[16], (size_t)n16 * 16);
    int8_t *d_out = (int8_t *)buf_get(ctx, ms->buf[1], (size_t)(total ? total : 1));
    if (!d_work || !d_out)
        return sfe_set_err(ctx, SFE_ERR_HIP, "map set render2: scratch of %lld + %lld bytes failed", (long long)n16 * 16, total);
    for (size_t i = 0; i < marks.size(); ++i)
        marks[i].img = d_work + mark_work[i];
    const Render2Job *d_jobs = buf_stage(ctx, ms->buf[11], jobs);
    const MarkJob *d_marks = buf_stage(ctx, ms->buf[12], marks);
    const int32_t *d_spans = buf_stage(ctx, ms->buf[13], spans);
    // the host route's points: float64, float32 + keep flags; the store route's: frame lists, multiplicities + keep flags
    const double2 *d_xy = nullptr;
    float2 *d_xy32 = nullptr;
    const int32_t *d_frames = nullptr;
    int32_t *d_mult = nullptr;
    uint8_t *d_keep = nullptr;
    if (src.store) {
        const std::vector<int32_t> lists(src.frames, src.frames + (src.frames ? src.frame_off[n] : 0));
        d_frames = buf_stage(ctx, ms->buf[17], lists);
        d_mult = (int32_t *)buf_get(ctx, ms->buf[18], (sizeof(int32_t) + 1) * (size_t)(n_pts ? n_pts : 1));
        if (!d_jobs || !d_marks || !d_spans || !d_frames || !d_mult)
            return sfe_set_err(ctx, SFE_ERR_HIP, "map set render2: table upload failed");
        d_keep = (uint8_t *)(d_mult + (n_pts ? n_pts : 1));
    } else {
        d_xy = (const double2 *)buf_upload(ctx, ms->buf[14], xy, 2 * (size_t)n_pts);
        d_xy32 = (float2 *)buf_get(ctx, ms->buf[15], (sizeof(float2) + 1) * (size_t)(n_pts ? n_pts : 1));
        if (!d_jobs || !d_marks || !d_spans || !d_xy || !d_xy32)
            return sfe_set_err(ctx, SFE_ERR_HIP, "map set render2: table / point upload failed");
        d_keep = (uint8_t *)(d_xy32 + (n_pts ? n_pts : 1));
    }
    const auto blocks = [](int64_t items) { return (unsigned)std::min<int64_t>((items + MAP_THREADS - 1) / MAP_THREADS, 1 << 20); };
    hipLaunchKernelGGL(map2_fill_kernel, dim3(blocks(n16)), dim3(MAP_THREADS), 0, ctx->stream, (uint4 *)d_work, n16);
    SFE_LAUNCH_CHECK(ctx);
    if (!marks.empty()) {
        hipLaunchKernelGGL(map2_mark_kernel, dim3(blocks(max_px), (unsigned)marks.size()), dim3(MAP_THREADS), 0, ctx->stream,
                           d_marks);
        SFE_LAUNCH_CHECK(ctx);
    }
    if (n_pts) {
        const dim3 rows((unsigned)((max_pts + 255) / 256), (unsigned)n); // a block per 256 points of every job's cloud
        const float2 *d_pool = src.store ? (const float2 *)v.d_pool : nullptr;
        if (src.store) {
            hipLaunchKernelGGL(map2_select_kernel, rows, dim3(256), 0, ctx->stream, d_jobs, v.d_key, d_frames, d_mult, d_keep);
            SFE_LAUNCH_CHECK(ctx);
            if (any_filter) {
                hipLaunchKernelGGL(map2_radius_count_store_kernel, rows, dim3(256), 0, ctx->stream, d_jobs, d_pool,
                                   (const int32_t *)d_mult, d_keep);
                SFE_LAUNCH_CHECK(ctx);
            }
        } else {
            hipLaunchKernelGGL(map2_cast_kernel, dim3(blocks(n_pts)), dim3(MAP_THREADS), 0, ctx->stream, d_xy, n_pts, d_xy32,
                               d_keep);
            SFE_LAUNCH_CHECK(ctx);
            if (any_filter) {
                hipLaunchKernelGGL(map2_radius_count_kernel, rows, dim3(256), 0, ctx->stream, d_jobs, (const float2 *)d_xy32,
                                   d_keep);
                SFE_LAUNCH_CHECK(ctx);
            }
        }
        hipLaunchKernelGGL(map2_stamp_kernel, dim3(blocks(max_stamp), (unsigned)n), dim3(MAP_THREADS), 0, ctx->stream, d_jobs,
                           d_xy, (const float2 *)d_xy32, d_pool, (const uint8_t *)d_keep, d_spans, d_work);
        SFE_LAUNCH_CHECK(ctx);
    }
    if (max_out) {
        hipLaunchKernelGGL(map2_resize_kernel, dim3(blocks(max_out), (unsigned)n), dim3(MAP_THREADS), 0, ctx->stream, d_jobs,
                           (const int8_t *)d_work, d_out);
        SFE_LAUNCH_CHECK(ctx);
        // (bytes of `total` no job covers are whatever the scratch held: the offsets are the caller's)
        SFE_HIP(ctx, hipMemcpyAsync(occ_out, d_out, (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
    }
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (and xy may go away)
    return 0;
}

int sfe_mapset_render2(sfe_mapset *ms, int n, const int32_t *maps, const int32_t *slot_off, const int32_t *slots,
                       const int32_t *box4, const int32_t *pt_off, const double *xy, const int32_t *filter,
                       const double *radius, const int32_t *min_points, const int32_t *dilate_hs, const double *origin2,
                       const double *resolution, const int32_t *out_hw, const double *inv, const int32_t *resize,
                       const long long *out_off, int8_t *occ_out, long long total)
{
    Render2Src src;
    src.pt_off = pt_off, src.xy = xy;
    return set_render2(ms, src, n, maps, slot_off, slots, box4, filter, radius, min_points, dilate_hs, origin2, resolution,
                       out_hw, inv, resize, out_off, occ_out, total);
}

// sfe_mapset_render2 with job b's points taken from cloud handles[b] of `store`, in place (sonarfe.h)
int sfe_mapset_render2_store(sfe_mapset *ms, sfe_cloud_store *store, int n, const int32_t *maps, const int32_t *slot_off,
                             const int32_t *slots, const int32_t *box4, const int32_t *handles, const int32_t *all_frames,
                             const int32_t *frame_off, const int32_t *frames, const int32_t *filter, const double *radius,
                             const int32_t *min_points, const int32_t *dilate_hs, const double *origin2,
                             const double *resolution, const int32_t *out_hw, const double *inv, const int32_t *resize,
                             const long long *out_off, int8_t *occ_out, long long total)
{
    if (!ms)
        return SFE_ERR_ARG;
    SFE_ARG(ms->ctx, store);
    Render2Src src;
    src.store = store, src.handles = handles, src.all_frames = all_frames, src.frame_off = frame_off, src.frames = frames;
    return set_render2(ms, src, n, maps, slot_off, slots, box4, filter, radius, min_points, dilate_hs, origin2, resolution,
                       out_hw, inv, resize, out_off, occ_out, total);
}

int sfe_mapset_hit_table(sfe_mapset *ms, const float *bearings, int num_bearings, const double *breaks, const double *coef,
                         int n_intervals, double margin, int num_ranges, double range_resolution, int range_in_double,
                         int r_skip, int c_skip, int *id_out)
{
    if (!ms)
        return SFE_ERR_ARG;
    sfe_ctx *ctx = ms->ctx;
    if (int rc = sfe_use(ctx))
        return rc;
    SFE_ARG(ctx, bearings && breaks && coef && id_out && num_bearings >= 2 && n_intervals >= 1 && n_intervals < (1 << 20));
    SFE_ARG(ctx, margin > 0 && num_ranges >= 1 && range_resolution > 0 && r_skip >= 1 && c_skip >= 1);
    for (int k = 0; k < n_intervals; ++k)
        SFE_ARG(ctx, breaks[k] < breaks[k + 1]);
    SFE_ARG(ctx, breaks[0] <= (double)bearings[0] && (double)bearings[num_bearings - 1] <= breaks[n_intervals]);
    SFE_ARG(ctx, bearings[0] < bearings[num_bearings - 1]);
    HitTab t;
    double *d = nullptr;
    const size_t nb = (size_t)n_intervals + 1, nc = 4 * (size_t)n_intervals;
    SFE_HIP(ctx, hipMalloc((void **)&d, sizeof(double) * (nb + nc)));
    if (hipMemcpy(d, breaks, sizeof(double) * nb, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d + nb, coef, sizeof(double) * nc, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        return sfe_set_err(ctx, SFE_ERR_HIP, "map hit table upload failed");
    }
    t.breaks = d, t.coef = d + nb;
    t.n_iv = n_intervals, t.num_ranges = num_ranges, t.num_bearings = num_bearings, t.r_skip = r_skip, t.c_skip = c_skip;
    t.wide = range_in_double ? 1 : 0;
    t.res32 = (float)range_resolution, t.res64 = range_resolution;
    t.b_first = (double)bearings[0], t.b_last = (double)bearings[num_bearings - 1], t.margin = margin;
    ms->hit_tabs.push_back(t);
    *id_out = (int)ms->hit_tabs.size() - 1;
    return 0;
}

// Phase one of a store-fed measurement (sonarfe.h).  Nothing of the set has changed when this returns, pending or not.
int sfe_mapset_measure_store(sfe_mapset *ms, sfe_cloud_store *store, int n, const int32_t *maps, const int32_t *slots,
                             const int32_t *geoms, const int32_t *handles, const int32_t *tabs, double radius, int min_points,
                             const int32_t *hrhc, const int32_t *k_off, const float *ktab, int n_ktab, const double *div,
                             float miss32, float logit_miss, float hit32, float logit_hit, int32_t *n_points_out,
                             int32_t *n_undecided_out)
{
    if (!ms)
        return SFE_ERR_ARG;
    sfe_ctx *ctx = ms->ctx;
    if (int rc = sfe_use(ctx))
        return rc;
    SFE_ARG(ctx, n <= 0 || maps);
    SFE_ARG(ctx, store && sfe_store_ctx(store) == ctx && n >= 0 && n <= 65535 && n_ktab >= 0 && (n_ktab == 0 || ktab));
    SFE_ARG(ctx, n == 0 || (slots && geoms && handles && tabs && hrhc && k_off && div && n_points_out && n_undecided_out));
    SFE_ARG(ctx, min_points <= 1 || radius >= 0);
    FeedState &f = ms->feed;
    f.pending = false;
    if (n == 0)
        return 0;
    SfeStoreView v;
    if (int rc = sfe_store_view(store, &v))
        return rc;
    std::vector<MeasJob> jobs(n);
    std::vector<FeedJob> fjobs(n);
    std::vector<std::pair<int32_t, int32_t>> named(n);
    int64_t px = 0, tot = 0;
    int max_n = 0;
    for (int b = 0; b < n; ++b) {
        MeasJob &j = jobs[b];
        if (int rc = set_slot_check(ms, maps[b], slots[b], geoms[b]))
            return rc;
        named[b] = {maps[b], slots[b]};
        const MapGeom &g = ms->geoms[geoms[b]];
        j.img_rows = g.img_rows, j.img_cols = g.img_cols, j.slot_px = g.img_rows * g.img_cols;
        j.logodds = nullptr; // feed_finish binds the slot
        const int hd = handles[b];
        if (hd < 0 || hd >= v.n_slots || v.cnt[hd] < 0)
            return sfe_set_err(ctx, SFE_ERR_ARG, "map set: cloud %d named (job %d), the store holds %d%s", hd, b, v.n_slots,
                               (hd >= 0 && hd < v.n_slots) ? " and that one was not stored" : "");
        SFE_ARG(ctx, tabs[b] >= 0 && tabs[b] < (int)ms->hit_tabs.size());
        const int cnt = v.cnt[hd];
        j.hit_off = (int32_t)tot;
        j.n_hits = cnt;
        // a cloud without points is a keyframe without a measurement (hr < 0); one the filter empties keeps its kernel
        j.hr = cnt ? hrhc[2 * b] : -1, j.hc = cnt ? hrhc[2 * b + 1] : 0;
        j.k_off = cnt ? k_off[b] : 0;
        j.div = cnt ? div[b] : 1.0;
        SFE_ARG(ctx, j.hr < 1024 && j.hc < 1024 && (j.hr < 0 || j.hc >= 0));
        SFE_ARG(ctx, cnt == 0 || (j.hr >= 0 && j.k_off >= 0 && (int64_t)j.k_off + (2 * j.hr + 1) * (2 * j.hc + 1) <= n_ktab));
        j.px_off = px;
        px += j.slot_px;
        fjobs[b].off = v.off[hd], fjobs[b].n = cnt, fjobs[b].hit_off = (int32_t)tot, fjobs[b].tab = tabs[b];
        tot += cnt;
        max_n = max(max_n, cnt);
        SFE_ARG(ctx, tot < (1 << 30));
    }
    std::sort(named.begin(), named.end());
    SFE_ARG(ctx, std::adjacent_find(named.begin(), named.end()) == named.end()); // a slot holds one image
    FeedJob *d_jobs = buf_stage(ctx, ms->buf[6], fjobs);
    HitTab *d_tabs = buf_stage(ctx, ms->buf[10], ms->hit_tabs);
    int32_t *d_hits = (int32_t *)buf_get(ctx, ms->buf[7], sizeof(int32_t) * 2 * (size_t)(tot + 1));
    uint8_t *d_keep = (uint8_t *)buf_get(ctx, ms->buf[8], (size_t)(tot + 1));
    char *d_und = (char *)buf_get(ctx, ms->buf[9], sizeof(UndPoint) * (size_t)tot + sizeof(int32_t) * (size_t)n);
    int32_t *h_cnt = (int32_t *)sfe_pinned_io(ctx, 3, sizeof(int32_t) * (size_t)n);
    if (!d_jobs || !d_tabs || !d_hits || !d_keep || !d_und || !h_cnt)
        return sfe_set_err(ctx, SFE_ERR_HIP, "map set store feed scratch allocation / upload failed");
    int32_t *d_cnt = (int32_t *)(d_und + sizeof(UndPoint) * (size_t)tot);
    SFE_HIP(ctx, hipMemsetAsync(d_cnt, 0, sizeof(int32_t) * (size_t)n, ctx->stream));
    if (max_n > 0) {
        const dim3 grid((unsigned)((max_n + 255) / 256), (unsigned)n);
        const bool filter = min_points > 1; // Mapping._hits
        if (filter) {
            hipLaunchKernelGGL(feed_radius_count_kernel, grid, dim3(256), 0, ctx->stream, (const float2 *)v.d_pool, d_jobs,
                               (float)(radius * radius), min_points, d_keep);
            SFE_LAUNCH_CHECK(ctx);
        }
        hipLaunchKernelGGL(feed_hit_cells_kernel, grid, dim3(256), 0, ctx->stream, (const float2 *)v.d_pool, d_jobs, d_tabs,
                           filter ? (const uint8_t *)d_keep : nullptr, d_hits, (UndPoint *)d_und, d_cnt);
        SFE_LAUNCH_CHECK(ctx);
    }
    SFE_HIP(ctx, hipMemcpyAsync(h_cnt, d_cnt, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    f.maps.assign(maps, maps + n), f.slots.assign(slots, slots + n), f.geoms.assign(geoms, geoms + n);
    f.n_und.assign(h_cnt, h_cnt + n);
    f.jobs = jobs;
    f.ktab.assign(ktab, ktab + n_ktab);
    f.miss32 = miss32, f.logit_miss = logit_miss, f.hit32 = hit32, f.logit_hit = logit_hit;
    f.tot = (int)tot, f.tot_und = 0;
    for (int b = 0; b < n; ++b) {
        n_points_out[b] = jobs[b].n_hits;
        n_undecided_out[b] = h_cnt[b];
        f.tot_und += h_cnt[b];
    }
    f.pending = true; // until the measurement runs: at once if no point is undecided
    return f.tot_und == 0 ? feed_finish(ms) : 0;
}

int sfe_mapset_measure_store_undecided(sfe_mapset *ms, float *xy_out, int32_t *pos_out, int cap)
{
    if (!ms)
        return SFE_ERR_ARG;
    if (int rc = sfe_use(ms->ctx))
        return rc;
    return feed_undecided(ms, xy_out, pos_out, cap);
}

int sfe_mapset_measure_store_finish(sfe_mapset *ms, int n_cells, const int32_t *pos, const int32_t *cells)
{
    if (!ms)
        return SFE_ERR_ARG;
    if (int rc = sfe_use(ms->ctx))
        return rc;
    if (int rc = feed_fill(ms, n_cells, pos, cells))
        return rc;
    return feed_finish(ms);
}

// ---- sfe_map: a set of one map with its slots on demand.  Every call is the set's over map 0 (sonarfe.h) ----------------

int sfe_map_create(sfe_ctx *ctx, int rows, int cols, sfe_map **out)
{
    if (int rc = sfe_use(ctx))
        return rc;
    return set_create(ctx, 1, rows, cols, 0, 0, reinterpret_cast<sfe_mapset **>(out));
}

void sfe_map_destroy(sfe_map *m) { sfe_mapset_destroy(one(m)); }

int sfe_map_geometry(sfe_map *m, const float *sonar_xy, int img_rows, int img_cols, int *id_out)
{
    return sfe_mapset_geometry(one(m), sonar_xy, img_rows, img_cols, id_out);
}

int sfe_map_set_logodds(sfe_map *m, int slot, int geom, const float *logodds)
{
    const int32_t map = 0, s = slot, g = geom;
    return sfe_mapset_set_logodds(one(m), 1, &map, &s, &g, logodds);
}

int sfe_map_measure(sfe_map *m, int n, const int32_t *slots, const int32_t *geoms, const int32_t *hit_off,
                    const int32_t *hits, const int32_t *hrhc, const int32_t *k_off, const float *ktab, int n_ktab,
                    const double *div, float miss32, float logit_miss, float hit32, float logit_hit)
{
    return sfe_mapset_measure(one(m), n, map0(n).data(), slots, geoms, hit_off, hits, hrhc, k_off, ktab, n_ktab, div, miss32,
                              logit_miss, hit32, logit_hit);
}

int sfe_map_measure_stages(sfe_map *m, int b, uint8_t *hits_out, float *prob_out, int32_t *first_hits_out)
{
    return sfe_mapset_measure_stages(one(m), b, hits_out, prob_out, first_hits_out);
}

int sfe_map_hit_table(sfe_map *m, const float *bearings, int num_bearings, const double *breaks, const double *coef,
                      int n_intervals, double margin, int num_ranges, double range_resolution, int range_in_double, int r_skip,
                      int c_skip, int *id_out)
{
    return sfe_mapset_hit_table(one(m), bearings, num_bearings, breaks, coef, n_intervals, margin, num_ranges, range_resolution,
                                range_in_double, r_skip, c_skip, id_out);
}

int sfe_map_measure_store(sfe_map *m, sfe_cloud_store *store, int n, const int32_t *slots, const int32_t *geoms,
                          const int32_t *handles, const int32_t *tabs, double radius, int min_points, const int32_t *hrhc,
                          const int32_t *k_off, const float *ktab, int n_ktab, const double *div, float miss32,
                          float logit_miss, float hit32, float logit_hit, int32_t *n_points_out, int32_t *n_undecided_out)
{
    return sfe_mapset_measure_store(one(m), store, n, map0(n).data(), slots, geoms, handles, tabs, radius, min_points, hrhc,
                                    k_off, ktab, n_ktab, div, miss32, logit_miss, hit32, logit_hit, n_points_out,
                                    n_undecided_out);
}

int sfe_map_measure_store_undecided(sfe_map *m, float *xy_out, int32_t *pos_out, int cap)
{
    return sfe_mapset_measure_store_undecided(one(m), xy_out, pos_out, cap);
}

int sfe_map_measure_store_finish(sfe_map *m, int n_cells, const int32_t *pos, const int32_t *cells)
{
    return sfe_mapset_measure_store_finish(one(m), n_cells, pos, cells);
}

int sfe_map_fit_bounds(sfe_map *m, int n, const int32_t *slots, const double *pose4, const double *origin2,
                       double resolution, int32_t *mm_out)
{
    return sfe_mapset_fit_bounds(one(m), n, map0(n).data(), slots, pose4, origin2, resolution, mm_out);
}

int sfe_map_grow(sfe_map *m, int top, int bottom, int left, int right)
{
    const int32_t map = 0, grow4[4] = {top, bottom, left, right};
    return sfe_mapset_grow(one(m), 1, &map, grow4);
}

int sfe_map_refit(sfe_map *m, int n, const int32_t *slots, const double *pose4, const double *origin2, double resolution,
                  const int32_t *mm, const int32_t *shift2, const uint8_t *dec)
{
    return sfe_mapset_refit(one(m), n, map0(n).data(), slots, pose4, origin2, resolution, mm, shift2, dec);
}

int sfe_map_cells(sfe_map *m, int slot, uint16_t *r_out, uint16_t *c_out, float *l_out, int cap, int *n_out)
{
    return sfe_mapset_cells(one(m), 0, slot, r_out, c_out, l_out, cap, n_out);
}

int sfe_map_logodds(sfe_map *m, int slot, float *out, int cap) { return sfe_mapset_logodds(one(m), 0, slot, out, cap); }

int sfe_map_shape(sfe_map *m, int32_t *rows_cols_grow4) { return sfe_mapset_shape(one(m), 0, rows_cols_grow4); }

int sfe_map_read_grid(sfe_map *m, int which, float *out, long long cap)
{
    return sfe_mapset_read_grid(one(m), 0, which, out, cap);
}

int sfe_map_frames(sfe_map *m, int n, const int32_t *slots)
{
    const int32_t map = 0, slot_off[2] = {0, n};
    return sfe_mapset_frames(one(m), 1, &map, slot_off, slots);
}

int sfe_map_render(sfe_map *m, int which, int r0, int r1, int c0, int c1, int out_h, int out_w, double inv, int resize,
                   int8_t *occ_out)
{
    const int32_t map = 0, w = which, box4[4] = {r0, r1, c0, c1}, out_hw[2] = {out_h, out_w}, rs = resize;
    const long long out_off = 0;
    return sfe_mapset_render(one(m), 1, &map, &w, box4, out_hw, &inv, &rs, &out_off, occ_out, (long long)out_h * out_w);
}

int sfe_map_render2(sfe_map *m, int n_slots, const int32_t *slots, int r0, int r1, int c0, int c1, const double *xy, int n_pts,
                    int filter, double radius, int min_points, int dilate_hs, double y0, double x0, double resolution,
                    int out_h, int out_w, double inv, int resize, int8_t *occ_out)
{
    const int32_t map = 0, slot_off[2] = {0, n_slots}, box4[4] = {r0, r1, c0, c1}, pt_off[2] = {0, n_pts}, f = filter;
    const int32_t mp = min_points, hs = dilate_hs, out_hw[2] = {out_h, out_w}, rs = resize;
    const double origin2[2] = {y0, x0};
    const long long out_off = 0;
    return sfe_mapset_render2(one(m), 1, &map, slot_off, slots, box4, pt_off, xy, &f, &radius, &mp, &hs, origin2, &resolution,
                              out_hw, &inv, &rs, &out_off, occ_out, (long long)out_h * out_w);
}

int sfe_map_render2_store(sfe_map *m, sfe_cloud_store *store, int n_slots, const int32_t *slots, int r0, int r1, int c0, int c1,
                          int handle, int all_frames, const int32_t *frames, int n_frames, int filter, double radius,
                          int min_points, int dilate_hs, double y0, double x0, double resolution, int out_h, int out_w,
                          double inv, int resize, int8_t *occ_out)
{
    const int32_t map = 0, slot_off[2] = {0, n_slots}, box4[4] = {r0, r1, c0, c1}, frame_off[2] = {0, n_frames};
    const int32_t hd = handle, all = all_frames, f = filter, mp = min_points, hs = dilate_hs, out_hw[2] = {out_h, out_w};
    const double origin2[2] = {y0, x0};
    const long long out_off = 0;
    return sfe_mapset_render2_store(one(m), store, 1, &map, slot_off, slots, box4, &hd, &all, frame_off, frames, &f, &radius,
                                    &mp, &hs, origin2, &resolution, out_hw, &inv, &resize, &out_off, occ_out,
                                    (long long)out_h * out_w);
}

int sfe_map_enable_intensity(sfe_map *m) { return sfe_mapset_enable_intensity(one(m)); }

int sfe_map_set_intensity(sfe_map *m, int slot, int geom, int full_rows, int full_cols, int r_skip, int c_skip,
                          const uint8_t *image)
{
    const int32_t map = 0, s = slot, g = geom, shape4[4] = {full_rows, full_cols, r_skip, c_skip};
    return sfe_mapset_set_intensity(one(m), 1, &map, &s, &g, shape4, image);
}

int sfe_map_set_intensity_dev(sfe_map *m, int slot, int geom, int full_rows, int full_cols, int r_skip, int c_skip,
                              const void *d_image, long long row_stride)
{
    const int32_t map = 0, s = slot, g = geom, shape4[4] = {full_rows, full_cols, r_skip, c_skip};
    return sfe_mapset_set_intensity_dev(one(m), 1, &map, &s, &g, shape4, &d_image, &row_stride);
}

int sfe_map_render_intensity(sfe_map *m, int r0, int r1, int c0, int c1, int8_t *out)
{
    const int32_t map = 0, box4[4] = {r0, r1, c0, c1};
    const long long out_off = 0;
    return sfe_mapset_render_intensity(one(m), 1, &map, box4, &out_off, (long long)(r1 - r0 + 1) * (c1 - c0 + 1), out);
}

int sfe_map_read_intensity(sfe_map *m, uint32_t *intensity_out, uint16_t *counter_out, long long cap)
{
    return sfe_mapset_read_intensity(one(m), 0, intensity_out, counter_out, cap);
}

int sfe_map_slot_intensity(sfe_map *m, int slot, uint8_t *image_out, int image_cap, uint8_t *i_out, int cells_cap, int *n_out)
{
    return sfe_mapset_slot_intensity(one(m), 0, slot, image_out, image_cap, i_out, cells_cap, n_out);
}

int sfe_remove_outlier_many(sfe_ctx *ctx, const float *pts, const int32_t *off, int n_clouds, double radius, int min_points,
                            uint8_t *keep_out)
{
    if (int rc = sfe_use(ctx))
        return rc;
    SFE_ARG(ctx, n_clouds >= 0 && n_clouds <= 65535 && (n_clouds == 0 || off));
    if (n_clouds == 0)
        return 0;
    int max_n = 0;
    SFE_ARG(ctx, off[0] == 0);
    for (int c = 0; c < n_clouds; ++c) {
        SFE_ARG(ctx, off[c + 1] >= off[c]);
        max_n = max(max_n, off[c + 1] - off[c]);
    }
    const int n = off[n_clouds];
    if (n == 0)
        return 0;
    SFE_ARG(ctx, pts && keep_out);
    float *d_pts = (float *)sfe_scratch(ctx, 0, sizeof(float) * 2 * (size_t)n);
    uint8_t *d_keep = (uint8_t *)sfe_scratch(ctx, 2, (size_t)n);
    int32_t *d_off = (int32_t *)sfe_scratch(ctx, 1, sizeof(int32_t) * ((size_t)n_clouds + 1));
    if (!d_pts || !d_keep || !d_off)
        return SFE_ERR_HIP;
    SFE_HIP(ctx, hipMemcpyAsync(d_pts, pts, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    SFE_HIP(ctx, hipMemcpyAsync(d_off, off, sizeof(int32_t) * ((size_t)n_clouds + 1), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(radius_count_many_kernel, dim3((unsigned)((max_n + 255) / 256), (unsigned)n_clouds), dim3(256), 0,
                       ctx->stream, (const float2 *)d_pts, d_off, (float)(radius * radius), min_points, d_keep);
    SFE_LAUNCH_CHECK(ctx);
    SFE_HIP(ctx, hipMemcpyAsync(keep_out, d_keep, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    SFE_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

} // extern "C"
