// Internal definitions shared by the libsonarfe translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/sonarfe.h"
#include "sfe_icp_gen.h"

#define SFE_NSCRATCH 81 // (0..71: the numbers and the CF_SLOT_* / DPF_SLOT_* / DPF3_SLOT_* names in the .hip files; 72..80: sfe_icp_sweep.hip)
#define SFE_ICP_PROF_N 96 // values sfe_icp_get_profile hands back

// Launcher knobs of one context, set by name with sfe_tune (the name -> field / range table is in sfe_ctx.hip).  The
// member initialisers are the shipped defaults; every setting computes the same results.
struct sfe_tuning {
    // CFAR, OS (sfe_cfar.hip)
    int cfar_os_gated = 1;      // behind a gate of at least cfar_os_gated_min: the candidates-only kernel (0: histogram)
    int cfar_os_gated_min = 40; //   (gate 65: 0.65 ms per 512 frames against the histogram's 1.65; gate 20: 1.84 against 1.65)
    int cfar_os_pref = 1;       // below it: the pre-filtered candidate kernel where it applies (0: sliding histogram)
    int cfar_os_pref_x = 80;    //   its level: L[x] for a pixel of about a third of full scale
    // extraction (sfe_extract.hip)
    int extract_rec_cap = 0;    // record slots per workgroup region of the record path (0: ME_THREADS x ME_RPT)
    int extract_capw = 0;       // canvas words a frame of the record path may fill (0: 4096)
    int extract_compact = 1;    // inverse map in its 4-byte entries (0: the 8-byte entries of round 3)
    // matching cost (sfe_cost.hip)
    int cost_many = 1;          // 32+ poses per job: 64 per workgroup around one staged grid (0: 8 per workgroup)
    // strip-sweep ICP (sfe_icp_sweep.hip)
    int sw_tiers = 1;           // one-wave / four-wave workgroups for small jobs (0: every job on 1024 threads)
    int sw_tiny = 1;            // clouds of a few hundred points: the exhaustive one-wave kernel
    int sw_multi = 1;           // large jobs shared by several workgroups (off too under sfe_icp_set_tuning bit 4 and in IcpCall::unsplit's retry)
    int sw_multi_g = 0;         //   shares per job (0: as many as the CUs allow, at most SW_MG_MAX)
    int sw_multi_min_src = 8192; //  fewest queries of a job that is shared
    int sw_multi_share_min = 1024; // fewest queries worth a share
    int sw_cache = 1;           // witness / clearance cache
    int sw_rec = 1;             // clearance records (long fixed-count chains only)
    int sw_budget = 128;        // second pass (all strips): trips + strips before a query goes to the cooperative tier
    int sw_budget_a = 6;        // first pass (own strip): walk trips (4 candidates each) before a query is handed on
    int sw_margin = 15;         // percent: the next iteration's cap over this iteration's limit
    int sw_rtrips = 4;          // second pass: walk trips between two chances to move on to the next strip
    int sw_recm = 8;            // percent: clearance records search this much further (radius; ~17 % more candidates)
    float sw_reck = 3.0f;       //   ... plus this many times the largest movement of the last step
    int sw_strip_pts = 96;      // target points per strip
    int sw_union_iters = 1;     // first iterations that scan the union of a wave's windows
    int sw_union_max = 768;     //   ... of at most this many points
    int icp_debug = 0;          // watchdogs of the sweep kernel reported on stderr (synchronises every call)
};

// CFAR (sfe_cfar.hip): what the last call with a threshold map checked and uploaded, so that a stream of equal calls does
// neither again
struct SfeCfarCache {
    struct Key {
        int alg = -1, T = -1;
        double tau = 0.0;
        bool is(int a, int t, double u) const { return alg == a && T == t && tau == u; }
    };
    Key arith;                     // cfar_thr_arith checked against the reference expression for these: arith_on
    int arith_on = 0;
    Key tab;                       // float threshold table of the sliding-sum kernel on the device at tab_ptr (scratch slot 37)
    const void *tab_ptr = nullptr;
};

struct sfe_ctx {
    int device = -1;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // side stream of the ICP launcher (icp_variant bit 3), created with the lowest priority the device offers: the
    // preparation of a batch whose inputs are final is enqueued here and takes the CUs that the kernels on `stream` --
    // the loop kernel of the batch before, mostly, and the front end of the same step -- leave free.  ev_prep
    // orders the loop kernel behind it.  What the preparation writes and the loop reads exists in two generations
    // (sfe_icp_gen.h); ev_loop[g] is recorded behind the loop kernels that read generation g and keeps the
    // preparation of the batch after next off that scratch; ev_loop_begin is recorded in front of a batch's loop
    // kernels, and the next preparation starts behind it: next to a loop kernel, not next to the caller's other work.
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_prep = nullptr, ev_loop[2] = {nullptr, nullptr}, ev_loop_begin = nullptr;
    SfeIcpGenState icp_gens;
    // copy stream of the streamed-input path (sfe_memcpy_h2d_async): uploads from pinned host memory run next to the
    // kernels on `stream`; ev_copy = behind the last upload, ev_compute = where the kernels stood when the caller last
    // said "everything enqueued so far has consumed its input" (sfe_stream_fence)
    hipStream_t stream_copy = nullptr;
    hipEvent_t ev_copy = nullptr, ev_compute = nullptr;
    std::string err;
    struct Buf {
        void *p = nullptr;
        size_t cap = 0;
    } scratch[SFE_NSCRATCH];
    // pinned host staging for the small tables a launch hands to the device (job records, offsets): two blocks
    // used alternately, each guarded by the event recorded behind its last copy, so that enqueue-only (_dev)
    // entry points never synchronise a stream to keep a pageable vector alive
    struct Pin {
        void *p = nullptr;
        size_t cap = 0;
        hipEvent_t ev = nullptr;
        bool pending = false;
    } pin[2];
    int pin_next = 0;
    void *bm_clean_ptr = nullptr; // sfe_extract.hip (CleanBitmap): the canvas bitmap scratch is known to be zero up to bm_clean_bytes
    size_t bm_clean_bytes = 0;
    Pin pin_io[4]; // grow-only pinned buffers of the synchronous single-item entry points (no events: the call syncs)
    SfeCfarCache cfar_cache;
    int cfar_tile_rows = 0;
    int cfar_variant = 0;
    int icp_variant = 0;
    int extract_variant = 0;     // 0 = inverse map for binary masks, records instead of a canvas for bit-stream batches (default); 1 = dense pass only; 2 = inverse map through the canvas bitmap always (A/B)
    int icp_prof = 0;            // debug: per-phase cycle counts of workgroup 0 of the sweep kernel
    long long icp_prof_host[SFE_ICP_PROF_N] = {0};
    std::vector<int8_t> icp_routes; // SFE_ICP_ROUTE_* of every job of the last ICP call (sfe_icp_last_routes)
    int n_cu = 256;
    // clouds left in the staging slots by sfe_extract_points_bits_staged_dev, waiting for sfe_cloud_filter_staged_dev
    // (-1: none; anything else that writes those slots resets it)
    int staged_frames = -1;
    long long staged_cap = 0;
    sfe_tuning tune;
};

struct sfe_geom {
    sfe_ctx *ctx = nullptr;
    int cart_rows = 0, cart_cols = 0, polar_rows = 0, polar_cols = 0;
    double width = 0, height = 0;
    int32_t *d_code = nullptr;   // per Cartesian pixel: packed (iy, ix, table index) or -1
    int32_t *d_span = nullptr;   // per Cartesian row: [first, last+1) columns with code != -1
    int words_per_row = 0;       // 64-bit bitmap words per Cartesian row
    unsigned rcp = 0;            // ceil(2^32 / (polar_cols+1))
    int32_t *d_tile_rows = nullptr; // per canvas tile: [ylo, yhi] polar rows tapped by its valid pixels
    int word_groups = 0, tiles_per_frame = 0, lds_bytes = 0;
    // inverse map for sparse binary masks: for every polar pixel the canvas pixels that tap it with a
    // non-zero weight (CSR: offsets [polar_rows * polar_cols + 1], entries = linear canvas indices)
    int32_t *d_inv_off = nullptr;
    uint2 *d_inv_lut = nullptr;     // {canvas index, decision table of the entry} (extract_gather_kernel)
    uint2 *d_inv_ob = nullptr;      // compact form (round 4): per polar pixel {offset into d_inv_c4, base bit index}
    uint32_t *d_inv_c4 = nullptr;   //   4-byte entries {table, tap place, dx, dy}, dead entries dropped
    // px -> m of feature_extraction.py:236-237 per canvas row / column (fp64, the reference's operation order,
    // evaluated once on the host: extract_expand_words_kernel looks the metres up instead of dividing per point)
    double *d_ytab = nullptr, *d_xtab = nullptr;
};

int sfe_set_err(sfe_ctx *ctx, int code, const char *fmt, ...);
int sfe_mask_pack(sfe_ctx *ctx, const uint8_t *d_mask, int n_frames, long long px, uint32_t *d_bits,
                  int32_t *d_nonbin); // sfe_extract.hip: byte mask -> bit stream
// grow-only device scratch; nullptr on failure.  Growing a slot frees its old block, so it first waits (host side) for
// all three streams of the context: no kernel of an earlier ICP batch, of either generation, still reads the block.
void *sfe_scratch(sfe_ctx *ctx, int slot, size_t bytes);
// Pinned staging: sfe_pinned_begin hands out a host block of >= bytes (waiting, if need be, for the copy that last
// read it -- two launches ago); the caller fills it, enqueues its hipMemcpyAsync calls on `s` and then calls
// sfe_pinned_end(ctx, s) so the block is not reused before those copies have run.  nullptr on failure.
void *sfe_pinned_begin(sfe_ctx *ctx, size_t bytes);
int sfe_pinned_end(sfe_ctx *ctx, hipStream_t s);
// grow-only pinned buffer `slot` (0..3) of >= bytes for entry points that end with a stream synchronisation
void *sfe_pinned_io(sfe_ctx *ctx, int slot, size_t bytes);

#define SFE_HIP(ctx, call)                                                                       \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return sfe_set_err((ctx), SFE_ERR_HIP, "%s failed: %s (%s:%d)", #call,               \
                               hipGetErrorString(e_), __FILE__, __LINE__);                       \
    } while (0)

#define SFE_LAUNCH_CHECK(ctx) SFE_HIP(ctx, hipGetLastError())

#define SFE_ARG(ctx, cond)                                                                       \
    do {                                                                                         \
        if (!(cond))                                                                             \
            return sfe_set_err((ctx), SFE_ERR_ARG, "bad argument: %s (%s:%d)", #cond, __FILE__,  \
                               __LINE__);                                                        \
    } while (0)

// What one ICP call carries beyond sfe_icp_params, handed from the entry point down to every launch (nothing of a call
// lives on the context).
struct IcpCall {
    sfe_icp_outliers ox = {}; // outlier filters / checker of a *_chain_ext call (all zero: none); the kernels take it by value
    bool unsplit = false;     // no job shared by several workgroups: the second run after SFE_ICP_SPLIT_TIMEOUT
};

// sfe_icp_sweep.hip: 0 = launched, 1 = a target exceeds the LDS capacity (use the brute-force kernel), < 0 = error
int sfe_icp_sweep_launch(sfe_ctx *ctx, const sfe_icp_params *p, const IcpCall &call, const float *d_src, const float *d_tgt,
                         const int32_t *jobs4, const float *d_guess9, int n_jobs, float *d_T9, int32_t *d_status,
                         int32_t *d_iters);

// sfe_icp.hip: the argument checks of a call's outlier settings (o == nullptr: none, passes)
int sfe_icp_check_outliers(sfe_ctx *ctx, const sfe_icp_outliers *o);
// ... one call with host guesses and host results on device pools and a validated job table (n_jobs x (src_start, n_src,
// tgt_start, n_tgt) in points): stages the guesses (or takes them where they are: d_guess9 != nullptr), launches, brings
// T / status / iterations back (one copy, one synchronisation) and, if a job reports SFE_ICP_SPLIT_TIMEOUT while sharing
// was on, launches once more unsplit.  iters may be nullptr.
int sfe_icp_run_host(sfe_ctx *ctx, const sfe_icp_params *p, IcpCall call, const float *d_src, const float *d_tgt,
                     const int32_t *jobs4, const float *guesses9, const float *d_guess9, int n_jobs, float *T_out9,
                     int32_t *status, int32_t *iters);
// sfe_icp_dpf.hip: the argument checks of a data-point filter chain, and sfe_icp_run_host behind the chain's filters: every
// distinct slice of the job table filtered once, the job table rebuilt on the filtered pools
int sfe_icp_dpf_check(sfe_ctx *ctx, const sfe_icp_dpf *st, int n);
int sfe_icp_dpf_run_host(sfe_ctx *ctx, const sfe_icp_params *p, const IcpCall &call, const sfe_icp_dpf *rd, int n_rd,
                         const sfe_icp_dpf *rf, int n_rf, const float *d_src, const float *d_tgt, const int32_t *jobs4,
                         const float *guesses9, int n_jobs, float *T_out9, int32_t *status, int32_t *iters);

// sfe_icp3.hip: the parameter check of the 3-D ICP (minimizer 0, or 2 / 3 with their normals_knn), and one 3-D ICP call on device pools of packed
// float triples with a validated job table (n_jobs x (src_start, n_src, tgt_start, n_tgt) in points, every cloud non-empty
// and inside its pool), host guesses (16 floats per job) and host results; one synchronisation.  iters may be nullptr.
// `o` (nullable; all zero: none): the MinDist / MedianDist / Bound modules, which pick the EXT build of the job kernel.
int sfe_icp3_check_params(sfe_ctx *ctx, const sfe_icp_params *p);
int sfe_icp3_run_dev(sfe_ctx *ctx, const sfe_icp_params *p, const sfe_icp_outliers *o, const float *d_src,
                     const float *d_tgt, const int64_t *jobs4, const float *guesses16, int n_jobs, float *T_out16,
                     int32_t *status, int32_t *iters);
// sfe_icp3_dpf.hip: the argument checks of a 3-D chain's modules and stages (no launch), and sfe_icp3_run_dev behind the
// chain's data-point filters: every distinct slice of the job table filtered once, the job table rebuilt on the filtered
// pools (context scratch).  Without stages it is sfe_icp3_run_dev.
int sfe_icp3_check_chain(sfe_ctx *ctx, const sfe_icp_outliers *o, const sfe_icp_dpf *rd, int n_rd, const sfe_icp_dpf *rf,
                         int n_rf);
int sfe_icp3_chain_run_dev(sfe_ctx *ctx, const sfe_icp_params *p, const sfe_icp_outliers *o, const sfe_icp_dpf *rd, int n_rd,
                           const sfe_icp_dpf *rf, int n_rf, const float *d_src, const float *d_tgt, const int64_t *jobs4,
                           const float *guesses16, int n_jobs, float *T_out16, int32_t *status, int32_t *iters);

// sfe_store.hip: append n_frames clouds ([f][cap] float2 + counts[f], device) to a store; enqueue only
struct sfe_cloud_store;
int sfe_store_append_dev(sfe_cloud_store *s, const int64_t *stamps, const float *d_clouds, const int32_t *d_counts,
                         int n_frames, int64_t cap, int flags, int32_t *handles_out);
// ... the count its commit wrote for a slot (< 0: SFE_STORE_*), copied in stream order to pinned memory; the store's context
int sfe_store_slot_count_async(sfe_cloud_store *s, int32_t handle, int32_t *h_pinned);
sfe_ctx *sfe_store_ctx(sfe_cloud_store *s);

// what a store is made of, for the other translation units that read clouds by handle (sfe_cost.hip); syncs the host
// mirror of the slot table first
struct SfeStoreView {
    const void *d_pool;     // float2 points
    const int64_t *d_off;   // device slot table
    const int32_t *d_cnt;
    const int64_t *off;     // host mirror (valid for slots < n_slots)
    const int32_t *cnt;
    int n_slots;
    const int32_t *d_key;   // a key per pool point, for the keyed slots (nullptr: no slot is keyed yet)
    const uint8_t *keyed;   // host, n_keyed entries: the slot was built by a keyed entry point
    int n_keyed;
};
int sfe_store_view(sfe_cloud_store *s, SfeStoreView *v);

// sfe_cost.hip: cv2.getStructuringElement(MORPH_ELLIPSE, (2h+1, 2h+1)) as row spans: row i of the element covers columns
// [span[2 i], span[2 i + 1])
std::vector<int32_t> cost_ellipse_spans(int dilate_hs);

// sfe_downsample.hip: pcl.downsample with indices on a device-resident cloud of any size (rank sort in global memory)
struct SfeDsHeader {
    float cx, cy, radius;
    int levels;
    int n_seg;
};
int sfe_ds_run_dev(sfe_ctx *ctx, const float *d_pts, int n, float resolution, float *d_out, int32_t *d_out_idx,
                   SfeDsHeader *d_hdr);
int sfe_ds_run_dev_many(sfe_ctx *ctx, const float *d_pts, int n_jobs, const int32_t *d_n, int n_max, int stride,
                        float resolution, float *d_out, int32_t *d_out_idx, SfeDsHeader *d_hdr, int32_t *d_counts);

static inline int sfe_use(sfe_ctx *ctx)
{
    if (!ctx)
        return SFE_ERR_ARG;
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess)
        return sfe_set_err(ctx, SFE_ERR_HIP, "hipSetDevice(%d): %s", ctx->device, hipGetErrorString(e));
    return 0;
}
