/*
 * sonarfe.h -- C ABI of libsonarfe.so, the MI355X (gfx950) sonar front-end.
 *
 * This is the drop-in boundary for the two pybind11 modules of the reference
 * (there is no C ABI in the reference; these entry points are what a ctypes /
 * cgo / JNI binding of that path binds instead):
 *
 *   bruce_slam.cfar  (bruce_slam/src/bruce_slam/cpp/cfar.cpp:194-204)
 *       ca/soca/goca/os, ca2/soca2/goca2/os2        -> sfe_cfar_u8 / sfe_cfar_f32
 *   bruce_slam.pcl   (bruce_slam/src/bruce_slam/cpp/pcl.cpp:176-214)
 *       match                                       -> sfe_match
 *       remove_outlier                              -> sfe_remove_outlier
 *       downsample (both overloads)                 -> sfe_downsample
 *       ... the three on N x 3 clouds                -> sfe_match3, sfe_remove_outlier3, sfe_downsample3
 *       ICP.loadFromYaml / compute / getCovariance  -> sfe_icp_* (params parsed host-side)
 *       ICP.compute on N x 3 clouds, 4 x 4 guesses  -> sfe_icp3_compute_jobs
 *   feature_extraction.py:223-238 (CFAR gate, cv2.remap, nonzero, px->m)
 *                                                   -> sfe_geom_*, sfe_remap_u8, sfe_extract_points
 *
 * Conventions
 *   - plain pointers and sizes only; images are row-major (C order, numpy default):
 *     rows = range bins, cols = beams.  Point clouds are N x 2 float32 row-major
 *     (N x 3 for the entry points whose name ends in 3 or begins with sfe_icp3).
 *     Transforms are 3 x 3 float32 row-major (Pose2 matrix); 4 x 4 for sfe_icp3_compute_jobs.
 *   - entry points without a _dev suffix take HOST pointers (they copy in, run the
 *     HIP kernels, copy out) and are what the Python shims call.  *_dev entry points
 *     take DEVICE pointers obtained from sfe_malloc and only enqueue work on the
 *     context's stream (call sfe_sync to wait).
 *   - return value: 0 = success; > 0 = ICP convergence-class status (see
 *     SFE_ICP_*; the reference turns these into (what(), guess)); < 0 = hard error
 *     (bad argument, HIP failure) with text in sfe_last_error().  There is no CPU
 *     fallback anywhere: without a gfx950 device every compute entry point fails.
 *   - the library reads a number of SFE_* environment variables that switch between measured alternatives of the same
 *     computation (every setting returns identical results).  They are measurement tools, not part of this interface:
 *     DESIGN.md, appendix A lists them.
 *   - one sfe_ctx = one device + one HIP stream + its scratch; a ctx is not
 *     re-entrant (the reference's pybind calls hold the GIL and its ICP object is
 *     stateful, SURVEY 8b "Threading"); use one ctx per worker thread/process.
 */
#ifndef SONARFE_H
#define SONARFE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sfe_ctx sfe_ctx;
typedef struct sfe_geom sfe_geom;

/* hard-error codes (negative) */
#define SFE_ERR_ARG (-1)
#define SFE_ERR_HIP (-2)
#define SFE_ERR_NODEV (-3)
#define SFE_ERR_CAP (-4) /* caller-provided output capacity too small */

/* CFAR variants (cfar.cpp:10,30,53,76) */
#define SFE_CFAR_CA 0
#define SFE_CFAR_SOCA 1
#define SFE_CFAR_GOCA 2
#define SFE_CFAR_OS 3

/* ICP convergence-class statuses; messages are libpointmatcher's what() strings */
#define SFE_ICP_OK 0
#define SFE_ICP_NO_OUTLIER 1 /* "no outlier to filter" */
#define SFE_ICP_NO_POINT 2   /* "ErrorMnimizer: no point to minimize" */
#define SFE_ICP_NAN_ROT 3    /* "abs rotation norm not a number" */
#define SFE_ICP_NAN_TRANS 4  /* "abs translation norm not a number" */
#define SFE_ICP_SINGULAR 5   /* point-to-plane normal system not positive definite */
#define SFE_ICP_SPLIT_TIMEOUT 6 /* *_dev entry points only: the workgroups sharing one large job were not resident together (sfe_icp_set_tuning bit 4) */
#define SFE_ICP_DPF_EMPTY 7     /* *_chain entry points: the job's reading or reference has no point left after its data-point filters */
#define SFE_ICP_DPF_DEPTH 8     /* *_chain entry points: an OctreeGridDataPointsFilter stage needs a tree deeper than 24 levels */
#define SFE_ICP_BOUND 9         /* *_chain_ext entry points: "limit out of bounds" (BoundTransformationChecker) */

/* ---- library / context ------------------------------------------------- */
const char *sfe_version(void);
int sfe_device_count(int *count);
int sfe_ctx_create(int device, sfe_ctx **out);
void sfe_ctx_destroy(sfe_ctx *ctx);
const char *sfe_last_error(sfe_ctx *ctx); /* ctx may be NULL: error of the last failed create */
int sfe_sync(sfe_ctx *ctx);
int sfe_device_name(sfe_ctx *ctx, char *buf, int cap);
/* Launcher knob `name` of this context := value; the old value goes to *previous (may be NULL).  Every
 * setting computes the same results: the knobs choose kernels and their launch shapes.  An unknown name,
 * a value outside the knob's range or a fraction for an integer knob fails with SFE_ERR_ARG and changes
 * nothing.  The names, defaults and ranges (LAB_NOTEBOOK.md, Appendix A):
 *   cfar_os_gated (1), cfar_os_gated_min (40), cfar_os_pref (1), cfar_os_pref_x (80)     OS CFAR kernels
 *   extract_rec_cap (0 = built-in), extract_capw (0 = built-in), extract_compact (1)    batched extraction
 *   cost_many (1)                                                                       matching cost
 *   sw_tiers, sw_tiny, sw_multi (1), sw_multi_g (0), sw_multi_min_src (8192),           strip-sweep ICP
 *   sw_multi_share_min (1024), sw_cache, sw_rec (1), sw_budget (128), sw_budget_a (6),
 *   sw_margin (15), sw_rtrips (4), sw_recm (8), sw_reck (3.0, a float), sw_strip_pts (96),
 *   sw_union_iters (1), sw_union_max (768), icp_debug (0) */
int sfe_tune(sfe_ctx *ctx, const char *name, double value, double *previous);

/* device memory on the ctx's device, for resident pipelines (*_dev entry points) */
int sfe_malloc(sfe_ctx *ctx, size_t bytes, void **dptr);
int sfe_free(sfe_ctx *ctx, void *dptr);
int sfe_memcpy_h2d(sfe_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int sfe_memcpy_d2h(sfe_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
int sfe_memset(sfe_ctx *ctx, void *dst_dev, int value, size_t bytes);

/* Streamed inputs (feature_extraction.py:196-217: every ping arrives from the host).  Pinned host memory and uploads on
 * the context's copy stream, next to the kernels on its main stream:
 *   sfe_memcpy_h2d_async  enqueue-only upload from a sfe_host_alloc block
 *   sfe_stream_fence(0)   kernels enqueued from now on wait for every upload enqueued so far
 *   sfe_stream_fence(1)   uploads enqueued from now on wait for every kernel enqueued so far (their input buffer is free)
 *   sfe_stream_fence(2)   the host waits for the uploads */
int sfe_host_alloc(sfe_ctx *ctx, size_t bytes, void **hptr);
int sfe_host_free(sfe_ctx *ctx, void *hptr);
int sfe_memcpy_h2d_async(sfe_ctx *ctx, void *dst_dev, const void *src_pinned, size_t bytes);
int sfe_stream_fence(sfe_ctx *ctx, int what);

/* debug: the first `bytes` of the library's scratch buffer `slot` (intermediate results of the kernels) */
int sfe_debug_read_scratch(sfe_ctx *ctx, int slot, void *dst_host, size_t bytes);

/* HIP-event stopwatch on the ctx's stream (used by bench.py for per-kernel time) */
int sfe_timer_start(sfe_ctx *ctx);
int sfe_timer_stop(sfe_ctx *ctx, float *elapsed_ms); /* records, syncs, returns ms */

/* ---- CFAR: replaces bruce_slam.cfar (cfar.cpp:10-192) ------------------- */
/*
 * img: rows x cols.  train_hs/guard_hs/tau/k as passed by CFAR.detect
 * (CFAR.py:35-40,123-127).  intensity_thr >= 0 fuses feature_extraction.py:224
 * (mask &= img > thr); pass -1 for the plain cfar.* result.  thr_out (nullable)
 * receives the float threshold map of the *2 variants (cfar.cpp:98-192).
 * k is only read for SFE_CFAR_OS and must satisfy 0 <= k < 2*train_hs.
 */
int sfe_cfar_u8(sfe_ctx *ctx, const uint8_t *img, int rows, int cols, int alg, int train_hs,
                int guard_hs, int k, double tau, int intensity_thr, uint8_t *mask_out,
                float *thr_out);
/* float images (the pybind caster accepts any numeric dtype): exact float-sum semantics */
int sfe_cfar_f32(sfe_ctx *ctx, const float *img, int rows, int cols, int alg, int train_hs,
                 int guard_hs, int k, double tau, uint8_t *mask_out, float *thr_out);
/* batched, device-resident: n_frames images of rows x cols back to back */
int sfe_cfar_u8_batch_dev(sfe_ctx *ctx, const uint8_t *d_img, int n_frames, int rows, int cols,
                          int alg, int train_hs, int guard_hs, int k, double tau,
                          int intensity_thr, uint8_t *d_mask, float *d_thr);
/* The same detections as a bit stream, the form the batched extraction consumes: per frame
 * SFE_BITS_WORDS(rows*cols) uint32 words, bit (iy*cols + ix) of the stream (LSB first) = mask[iy][ix],
 * the last word of a frame is padding and written as 0.  For the windows of the register-ring kernel and
 * cols % 32 == 0 the kernel stores the bits itself (the 0/1 byte mask of CFAR.detect, feature_extraction.py:223,
 * never exists in memory); every other call runs the byte kernels into scratch and packs them.
 * d_bits: n_frames * SFE_BITS_WORDS(rows*cols) words, 4-byte aligned. */
#define SFE_BITS_WORDS(px) (((px) + 31) / 32 + 1)
int sfe_cfar_u8_bits_batch_dev(sfe_ctx *ctx, const uint8_t *d_img, int n_frames, int rows, int cols,
                               int alg, int train_hs, int guard_hs, int k, double tau,
                               int intensity_thr, uint32_t *d_bits);
/* tuning / A-B knob for the ring kernel: output rows per thread (0 = default) and
 * variant (0 = auto, 1 = force generic kernel, 2 = force ring kernel with prefetch depth 4, 3 = ring kernel depth 13) */
int sfe_cfar_set_tuning(sfe_ctx *ctx, int tile_rows, int variant);

/* ---- polar -> Cartesian: feature_extraction.py:134-173,226-238 --------- */
/*
 * A geometry = the (map_x, map_y) pair generate_map_xy builds (float32,
 * cart_rows x cart_cols, host pointers) for a polar image of polar_rows x
 * polar_cols, plus the metric extent used by the px->m step (width, height in m).
 * Creation uploads the maps and pre-decodes OpenCV's fixed-point coordinates.
 */
int sfe_geom_create(sfe_ctx *ctx, const float *map_x, const float *map_y, int cart_rows,
                    int cart_cols, int polar_rows, int polar_cols, double width, double height,
                    sfe_geom **out);
void sfe_geom_destroy(sfe_geom *g);
/* cv2.remap(src, map_x, map_y, cv2.INTER_LINEAR) for a uint8 image (BORDER_CONSTANT 0) */
int sfe_remap_u8(sfe_ctx *ctx, sfe_geom *g, const uint8_t *src, uint8_t *dst);
/* the same on device pointers (enqueue only): d_src polar_rows x polar_cols, d_dst cart_rows x cart_cols */
int sfe_remap_u8_dev(sfe_ctx *ctx, sfe_geom *g, const uint8_t *d_src, uint8_t *d_dst);
/* cv2.applyColorMap(cv2.remap(src, map_x, map_y, cv2.INTER_LINEAR), colormap) in one pass: the publishable bgr8 feature
 * image of feature_extraction.py:226-228 (dst_bgr: cart_rows x cart_cols x 3, B G R per pixel; the _dev form needs it
 * 4-byte aligned).  Only cv2.COLORMAP_JET (2), the one the node uses.  sfe_colormap_lut: the 256 x 3 BGR table itself
 * (applyColorMap(x, 2)[..] == lut[x]).  OpenCV's table restated, parity unpinned. */
#define SFE_COLORMAP_JET 2
int sfe_colormap_lut(int colormap, uint8_t *lut_bgr);
int sfe_remap_u8_colormap(sfe_ctx *ctx, sfe_geom *g, const uint8_t *src, int colormap, uint8_t *dst_bgr);
int sfe_remap_u8_colormap_dev(sfe_ctx *ctx, sfe_geom *g, const uint8_t *d_src, int colormap, uint8_t *d_dst_bgr);
/*
 * remap(mask) -> np.nonzero -> px->m in one call (feature_extraction.py:231-238).
 * mask: polar_rows x polar_cols uint8 0/1 (host).  Outputs (host, nullable):
 * rc_out int64 [cap x 2] = (row, col) in row-major order, pts_out float64 [cap x 2] =
 * (y_forward, x_lateral) in metres.  *n_out = number of points (may exceed cap -> SFE_ERR_CAP).
 */
int sfe_extract_points(sfe_ctx *ctx, sfe_geom *g, const uint8_t *mask, int64_t cap,
                       int64_t *rc_out, double *pts_out, int64_t *n_out);
/* A-B knob of the extraction: 0 = binary masks go through the inverse map (walk the set polar pixels, evaluate only the
 * canvas pixels that tap them; default) -- bit-stream batches without a canvas bitmap in HBM (records merged in LDS), frames
 * beyond that path's capacities and byte masks through the canvas bitmap; 1 = dense pass over the whole canvas for every
 * frame (what non-binary masks take anyway); 2 = inverse map through the canvas bitmap for every frame.  Identical results. */
int sfe_extract_set_tuning(sfe_ctx *ctx, int variant);
/* device-resident batch: per frame f, points go to d_pts + f*cap*2 (float64), count to d_counts[f]
 * (count is the true number even if it exceeds cap; only the first cap points are stored) */
int sfe_extract_points_batch_dev(sfe_ctx *ctx, sfe_geom *g, const uint8_t *d_mask, int n_frames,
                                 int64_t cap, double *d_pts, int32_t *d_counts);
/* the same from the bit streams of sfe_cfar_u8_bits_batch_dev (polar_cols % 32 == 0 required) */
int sfe_extract_points_bits_batch_dev(sfe_ctx *ctx, sfe_geom *g, const uint32_t *d_bits, int n_frames,
                                      int64_t cap, double *d_pts, int32_t *d_counts);
/* The same, handing the clouds to the resident cloud filters without the float64 round trip (round 6): next to d_counts the
 * call leaves every frame's points as float32 pairs -- the float64 metres of feature_extraction.py:235-238 rounded once, the
 * cast pybind makes when `points` enters pcl.downsample (pcl.cpp:128-131) -- and the frame's bounding box in the context's
 * staging area, where sfe_cloud_filter_staged_dev (below) picks them up; it must be the next filter call on this context with
 * the same n_frames and cap (anything else that stages clouds in between makes it fail with SFE_ERR_ARG, never run on stale
 * data).  d_pts [n_frames][cap][2] float64 is still required: with want_points64 != 0 it receives every frame's points like
 * sfe_extract_points_bits_batch_dev; with 0 only the frames that leave the fast path land there (dense frames beyond its
 * per-frame capacities; their float32 form is made from it) and the rest of it is left untouched -- 8 instead of 24 bytes
 * written per point.  cap <= 65536 (the filters' limit).  Enqueue only. */
int sfe_extract_points_bits_staged_dev(sfe_ctx *ctx, sfe_geom *g, const uint32_t *d_bits, int n_frames,
                                       int64_t cap, double *d_pts, int want_points64, int32_t *d_counts);

/* ---- point clouds: replaces bruce_slam.pcl (pcl.cpp:54-74,161-212) ------ */
typedef struct sfe_icp_params {
    float matcher_max_dist;  /* KDTreeMatcher.maxDist (icp.yaml:9) */
    int use_max_dist_filter; /* MaxDistOutlierFilter listed (icp.yaml:12) */
    float max_dist_filter;   /*   .maxDist (icp.yaml:13) */
    int use_trimmed_filter;  /* TrimmedDistOutlierFilter listed (icp.yaml:14) */
    float trim_ratio;        /*   .ratio (icp.yaml:15) */
    int minimizer;           /* 0 PointToPointErrorMinimizer (icp.yaml:20), 1 2-D PointToPlane (icp.yaml:18-19, force2D: 1;
                              * N x 2 clouds only), 2 3-D PointToPlane (force2D: 0; N x 3 clouds only, sfe_icp3_*),
                              * 3 3-D PointToPlane {force4DOF: 1}: yaw and translation only (N x 3 clouds only, sfe_icp3_*) */
    int max_iter;            /* CounterTransformationChecker.maxIterationCount (icp.yaml:24) */
    int use_diff_checker;    /* DifferentialTransformationChecker listed (icp.yaml:25) */
    float min_diff_rot;      /*   .minDiffRotErr (icp.yaml:26) */
    float min_diff_trans;    /*   .minDiffTransErr (icp.yaml:27) */
    int smooth_len;          /*   .smoothLength (icp.yaml:28) */
    int normals_knn;         /* point-to-plane only: neighbours (incl. self) for PCA normals */
} sfe_icp_params;

/* pcl.match(ref, in, knn=1, max_dist) (pcl.cpp:161-174): ids int32 [n_in] (-1 = none),
 * d2 float [n_in] squared distance (inf = none).  Ties -> lowest reference index. */
int sfe_match(sfe_ctx *ctx, const float *ref, int n_ref, const float *in, int n_in, float max_dist,
              int32_t *ids, float *d2);
/* the same for knn >= 1 neighbours (pcl.cpp:161-174 hands knn to KDTreeMatcher): ids / d2 are [knn x n_in] row-major
 * (the IntMatrix / Matrix pybind returns), row j = the (j+1)-th nearest reference point in ascending (d2, index)
 * order; -1 / inf where fewer than j+1 reference points lie within max_dist. */
int sfe_match_knn(sfe_ctx *ctx, const float *ref, int n_ref, const float *in, int n_in, int knn, float max_dist,
                  int32_t *ids, float *d2);
/* The densities pcl.density_filter computes (pcl.cpp:76-126: libpointmatcher SurfaceNormalDataPointsFilter{knn,
 * keepDensities}): per point the knn nearest points incl. itself, density = knn / ((4/3) pi r^3), r = the largest
 * distance of a neighbour from the neighbours' mean.  knn > n is an error (libnabo refuses it).  The second stage of
 * the reference's function (MaxDensityDataPointsFilter: sequential, std::rand) stays on the host, see pcl.py. */
int sfe_knn_density(sfe_ctx *ctx, const float *pts, int n, int knn, float *dens_out);
/* pcl.remove_outlier(points, radius, min_points) (pcl.cpp:54-74): order preserved */
int sfe_remove_outlier(sfe_ctx *ctx, const float *pts, int n, double radius, int min_points,
                       float *out, int *n_out);
/* pcl.downsample(points, resolution) (pcl.cpp:128-159): libpointmatcher OctreeGridDataPointsFilter
 * (maxSizeByNode = resolution, medoid per leaf, leaves in depth-first order).  out: up to n points,
 * out_idx (nullable): their indices in the input (the descriptor overload gathers with them). */
int sfe_downsample(sfe_ctx *ctx, const float *pts, int n, float resolution, float *out,
                   int32_t *out_idx, int *n_out);
/* The five calls above on N x 3 clouds (pcl.cpp's functions are dimension-generic; the reference carries such clouds as
 * Keyframe.points3D): the same arguments, points as packed float[n][3] (12-byte stride, no padding).  The rules are the
 * 2-D rules with one more coordinate: d2 = ((dx dx + dy dy) + dz dz), every product and sum rounded to float; the
 * octree is 8-way (child bit2 = z > centre z) with 3 key bits per level, so a tree deeper than 21 levels is cut there
 * (the 2-D rank chain: 31).  A cloud with z = 0 gives the 2-D call's result.  Brute-force kernels, quadratic in the
 * cloud size.  The 3-D downsample always writes out_idx (required) and has no resident route.  3-D ICP is
 * sfe_icp3_compute_jobs, further down. */
int sfe_match3(sfe_ctx *ctx, const float *ref, int n_ref, const float *in, int n_in, float max_dist,
               int32_t *ids, float *d2);
int sfe_match_knn3(sfe_ctx *ctx, const float *ref, int n_ref, const float *in, int n_in, int knn, float max_dist,
                   int32_t *ids, float *d2);
int sfe_knn_density3(sfe_ctx *ctx, const float *pts, int n, int knn, float *dens_out);
int sfe_remove_outlier3(sfe_ctx *ctx, const float *pts, int n, double radius, int min_points,
                        float *out, int *n_out);
int sfe_downsample3(sfe_ctx *ctx, const float *pts, int n, float resolution, float *out,
                    int32_t *out_idx, int *n_out);
/* Surface normals of an N x 3 cloud (libpointmatcher's SurfaceNormalDataPointsFilter {knn, keepNormals}; the routine the
 * 3-D point-to-plane ICP runs on its targets, here on the cloud as given, not centred).  Host pointers, pts and normals_out
 * packed float[n][3], 2 <= knn <= 16.  For point i:
 *   neighbours  its k = min(knn, n) nearest points of the cloud, i itself included: d2 = fl(fl(fl(dx dx) + fl(dy dy)) +
 *               fl(dz dz)), no fma, in lexicographic (d2, index) order -- equal distances go to the lowest index (the order
 *               of sfe_match_knn3).  A point whose d2 is not below +inf (NaN or infinite coordinates on either side) is
 *               nobody's neighbour, so a neighbourhood may hold fewer than k points, or none.
 *   normal      in fp64 from the float coordinates, in neighbour order: m = the neighbours' mean, C = sum (u - m)(u - m)^T;
 *               the unit eigenvector of C's smallest eigenvalue by a cyclic Jacobi (pairs (0,1), (0,2), (1,2), at most 12
 *               sweeps, none once the off-diagonal squares are below 1e-36 of the diagonal's; sfe_icp3_plane.h), the
 *               lowest column among equal eigenvalues, rounded to float.  Its sign is the Jacobi's: nothing here
 *               depends on it.  Always finite and of unit length: C = 0 (k < 2, coincident points, an empty
 *               neighbourhood) gives (1, 0, 0); collinear points give some unit vector across the line. */
int sfe_normals3(sfe_ctx *ctx, const float *pts, int n, int knn, float *normals_out);
/* pcl.ICP.compute(source, target, guess) (pcl.cpp:198-212).  Returns SFE_ICP_* (>= 0) or a
 * hard error (< 0).  On a nonzero status T_out = guess (pcl.cpp:203,207-210). */
int sfe_icp_compute(sfe_ctx *ctx, const sfe_icp_params *p, const float *src, int n_src,
                    const float *tgt, int n_tgt, const float *guess9, float *T_out9, int *iters);
/* many guesses on one cloud pair: the loop of SLAM.compute_icp_with_cov (slam.py:346-358) */
int sfe_icp_compute_guesses(sfe_ctx *ctx, const sfe_icp_params *p, const float *src, int n_src,
                            const float *tgt, int n_tgt, const float *guesses9, int n_guesses,
                            float *T_out9, int32_t *status, int32_t *iters);
/* many INDEPENDENT scan pairs in one launch (the job farm's unit; host pointers): clouds concatenated,
 * job j = src[src_off[j]..src_off[j+1]) against tgt[tgt_off[j]..tgt_off[j+1]) with guess 9*j.  Per job:
 * T_out9 (= the guess on a nonzero status, like pcl.cpp:203,207-210), status (SFE_ICP_*), iterations. */
int sfe_icp_compute_pairs(sfe_ctx *ctx, const sfe_icp_params *p, const float *src, const int32_t *src_off,
                          const float *tgt, const int32_t *tgt_off, const float *guesses9, int n_jobs,
                          float *T_out9, int32_t *status, int32_t *iters);
/* the same with an explicit job table, so that jobs may SHARE clouds (many guesses on one pair, one target matched
 * against many sources: the loop of slam.py:346-358 and the job farm's chunks): src / tgt = all clouds back to
 * back (n_src_pts / n_tgt_pts points in total), jobs4 = n_jobs x (src_start, n_src, tgt_start, n_tgt) in points.
 * Jobs naming the same target slice share one target preparation (sort, strip table, normals). */
int sfe_icp_compute_jobs(sfe_ctx *ctx, const sfe_icp_params *p, const float *src, int n_src_pts, const float *tgt,
                         int n_tgt_pts, const int32_t *jobs4, const float *guesses9, int n_jobs, float *T_out9,
                         int32_t *status, int32_t *iters);
/* pcl.ICP.compute on N x 3 clouds with 4 x 4 guesses (PM::ICP::compute, pcl.cpp:198-212, is dimension-generic; the
 * reference carries such clouds as Keyframe.points3D): the chain of the shipped config/icp.yaml with its point-to-point
 * minimiser (sfe_icp_params with minimizer == 0) or with PointToPlaneErrorMinimizer {force2D: 0} (minimizer == 2, with
 * 2 <= normals_knn <= 16) or its 4-DoF form {force4DOF: 1} (minimizer == 3, the same normals_knn bound); minimizer == 1, the
 * 2-D form, is SFE_ERR_ARG here (3-D clouds take the point-to-point or a 3-D point-to-plane minimiser), like a job slice
 * that is empty or outside the clouds.  Every 2-D entry point (sfe_icp_compute*) answers minimizer 2 and 3 with SFE_ERR_ARG.
 * Host pointers, the job table of sfe_icp_compute_jobs; src / tgt packed float[n][3], guesses16 / T_out16 4 x 4 row-major
 * per job.  One workgroup per job, brute-force search (sfe_icp3.hip); jobs naming the same target slice share nothing.
 * The route record of the last 2-D call stays as it is.  Rules, restated from libpointmatcher (parity unpinned, like the
 * 2-D chain); where one also exists in 2-D it is the 2-D rule with one more coordinate, so that a job whose clouds have
 * z = 0 and whose guess embeds a 3 x 3 guess reports the 2-D job's status and iterations and its pose to rounding:
 *   frame     reference mean per axis: fp64 sum rounded to float; the reference is centred by a float subtraction.
 *             T0 = translate(-mean) * guess, every 4 x 4 product entry (((a0 b0 + a1 b1) + a2 b2) + a3 b3) with each
 *             product and sum rounded to float; r = T0 * source (the 3-term affine, same rounding); every iteration
 *             matches c = T_iter * r.  Result T = translate(+mean) * (T_iter * T0); on a nonzero status T = the guess
 *             and iterations are as run.
 *   matcher   exact 1-NN, d2 = ((dx dx + dy dy) + dz dz) rounded at every step, no fma; ties: the lowest reference
 *             index; a query with !(d2 <= fl(maxDist * maxDist)), NaN included, has no match (-1, inf).
 *   outliers  MaxDist: d2 <= fl(maxDist^2).  Trimmed: d2 <= the k-th smallest of the n finite d2, k = (unsigned)((float)n
 *             * ratio), n - 1 when ratio >= 1; none finite: SFE_ICP_NO_OUTLIER.  No pair kept: SFE_ICP_NO_POINT.
 *   minimiser over the kept pairs (p = moved source point, q = its centred reference point) the fp64 sums W, sum p, sum q,
 *             sum q p^T; mp = sum p / W, mq = sum q / W, H = sum q p^T - (sum q) mp^T; R = the proper rotation closest to
 *             H (U V^T of the SVD H = U S V^T, the column of U of the smallest singular value negated when det < 0;
 *             computed as the top eigenvector of Horn's 4 x 4 matrix by fp64 Jacobi sweeps, sfe_icp3_solve.h);
 *             t = mq - R mp.  The step is rounded to float once, T_iter = T_step * T_iter.  H of rank <= 1 (all kept
 *             pairs collinear) leaves R undetermined: some finite rotation comes back, no particular one.
 *   minimizer 2  the normals of every distinct target (by first point and size) of the call are taken once, in front of the
 *             job kernel, by the rule of sfe_normals3 on the CENTRED target (3 floats per point in device scratch).  Match,
 *             outlier filters and checkers are the ones above.  Per kept pair, with n the normal of q, all widened to
 *             fp64: c = p x n, F = (c, n), e = n . (p - q); the fp64 sums W += 1, A += F F^T (21 distinct entries),
 *             b -= F e.  W == 0: SFE_ICP_NO_POINT.  A x = b by a 6 x 6 Cholesky with the 2-D minimiser's rule: A00 > 0
 *             and every later pivot > 1e-10 x its diagonal entry, else SFE_ICP_SINGULAR (T = the guess).  r = x[0..2],
 *             t = x[3..5], R = Rodrigues' rotation by |r| about r / |r| (the identity for |r| == 0); T_step = [R t]
 *             rounded to float.  A planar target (every z = 0 cloud) has parallel normals and a rank-3 A: status 5, so
 *             z = 0 input does NOT reduce to the 2-D point-to-plane result.
 *   minimizer 3  libpointmatcher's force4DOF: 1 -- the step has yaw and translation only (roll and pitch are never estimated:
 *             a Pose2-plus-depth state takes them from the IMU).  Normals, match, outlier filters, e and the checkers are
 *             minimizer 2's.  Per kept pair c = p_x n_y - p_y n_x (the third component of minimizer 2's p x n),
 *             F = (c, n_x, n_y, n_z); the fp64 sums W += 1, A += F F^T (10 distinct entries), b -= F e: 15 sums.  W == 0:
 *             SFE_ICP_NO_POINT.  A x = b by a 4 x 4 Cholesky under the pivot rule above, else SFE_ICP_SINGULAR (T = the
 *             guess).  gamma = x[0], R = [[cos gamma, -sin gamma, 0], [sin gamma, cos gamma, 0], [0, 0, 1]] in fp64 (no
 *             small-angle form), t = x[1..3]; T_step = [R t] rounded to float.  So with a guess that rotates about z only,
 *             entries (0,2), (1,2), (2,0), (2,1) of every T are exactly 0 and (2,2) is exactly 1.  Rank: a target whose
 *             normals all have n_z = 0 leaves t_z free, one whose normals are all +-z leaves yaw, t_x and t_y free:
 *             status 5 for both.
 *   checkers  Counter as in 2-D.  Differential: the history holds T_iter's float rotation block and translation, the
 *             identity first (a sliding window of 64 entries); per step, in fp64 from those floats, the rotation error
 *             is 2 atan2(|vec(q_i conj(q_i-1))|, |w|) with q the quaternion of the block by Eigen's branch rule (trace
 *             > 0, else the largest diagonal entry), the translation error the norm of the difference; both averaged
 *             over smoothLength and compared as in 2-D; NaN: SFE_ICP_NAN_ROT / SFE_ICP_NAN_TRANS. */
int sfe_icp3_compute_jobs(sfe_ctx *ctx, const sfe_icp_params *p, const float *src, int n_src_pts, const float *tgt,
                          int n_tgt_pts, const int32_t *jobs4, const float *guesses16, int n_jobs, float *T_out16,
                          int32_t *status, int32_t *iters);
/* Data-point filters of a libpointmatcher ICP chain (readingDataPointsFilters / referenceDataPointsFilters), 2-D.
 * A stage keeps a point (x, y) when
 *   SFE_DPF_MAX_DIST     dim -1: sqrtf(x*x + y*y) < |f[0]|, dim 0 / 1: x / y < f[0]           (maxDist = f[0])
 *   SFE_DPF_MIN_DIST     dim -1: sqrtf(x*x + y*y) > |f[0]|, dim 0 / 1: |x| / |y| > |f[0]|     (minDist = f[0])
 *   SFE_DPF_BOUNDING_BOX (xMin < x < xMax && yMin < y < yMax) != remove_inside, f = xMin xMax yMin yMax (zMin zMax unused)
 *   SFE_DPF_OCTREE_GRID  OctreeGridDataPointsFilter {maxSizeByNode = f[0] > 0, samplingMethod: 3 (medoid),
 *                        maxPointByNode: 1}: exactly sfe_downsample(cloud, f[0]); clouds of <= 65536 points
 * (every product / sum rounded to float, correctly rounded sqrtf).  Kept points keep their order.  A
 * SurfaceNormalDataPointsFilter keeps every point and has no code here: it is sfe_icp_params.normals_knn. */
#define SFE_DPF_MAX_DIST 0
#define SFE_DPF_MIN_DIST 1
#define SFE_DPF_BOUNDING_BOX 2
#define SFE_DPF_OCTREE_GRID 3
#define SFE_DPF_MAX_STAGES 8 /* stages per side of a chain */
typedef struct sfe_icp_dpf {
    int kind;          /* SFE_DPF_* */
    int dim;           /* MAX_DIST / MIN_DIST: -1 (norm), 0 (x), 1 (y); the 3-D entry points (sfe_icp3_*) also take 2 (z) */
    int remove_inside; /* BOUNDING_BOX */
    float f[6];        /* the stage's thresholds, see above */
} sfe_icp_dpf;
/* Runs n_stages stages in order over n_clouds device-resident clouds, cloud c = d_pts[off[c] .. off[c+1]) (off: host,
 * n_clouds + 1 entries, in points).  The survivors of cloud c go to d_out back to back (cloud c after the survivors of
 * clouds 0 .. c-1; d_out holds off[n_clouds] points), their number to counts_out[c] (host; -1: an octree stage needed a
 * tree deeper than 24 levels, no points written).  One stream synchronisation. */
int sfe_icp_filter_clouds_dev(sfe_ctx *ctx, const sfe_icp_dpf *stages, int n_stages, const float *d_pts,
                              const int32_t *off, int n_clouds, float *d_out, int32_t *counts_out);
/* sfe_icp_compute_guesses / _pairs / _jobs with a chain's data-point filters: the reading stages run once on every
 * distinct source cloud (slice) of the call, the reference stages once on every distinct target cloud, each in its own
 * frame before any guess is applied; ICP then runs on the filtered clouds (routes chosen by the filtered sizes).  A job
 * whose filtered reading or reference is empty reports SFE_ICP_DPF_EMPTY, one whose octree is too deep
 * SFE_ICP_DPF_DEPTH, both with T = the guess and 0 iterations (sfe_icp_last_routes: -1); the other jobs are unaffected.
 * With no stages on either side these are the plain entry points. */
int sfe_icp_compute_guesses_chain(sfe_ctx *ctx, const sfe_icp_params *p, const sfe_icp_dpf *rd, int n_rd,
                                  const sfe_icp_dpf *rf, int n_rf, const float *src, int n_src, const float *tgt, int n_tgt,
                                  const float *guesses9, int n_guesses, float *T_out9, int32_t *status, int32_t *iters);
int sfe_icp_compute_pairs_chain(sfe_ctx *ctx, const sfe_icp_params *p, const sfe_icp_dpf *rd, int n_rd,
                                const sfe_icp_dpf *rf, int n_rf, const float *src, const int32_t *src_off, const float *tgt,
                                const int32_t *tgt_off, const float *guesses9, int n_jobs, float *T_out9, int32_t *status,
                                int32_t *iters);
int sfe_icp_compute_jobs_chain(sfe_ctx *ctx, const sfe_icp_params *p, const sfe_icp_dpf *rd, int n_rd,
                               const sfe_icp_dpf *rf, int n_rf, const float *src, int n_src_pts, const float *tgt,
                               int n_tgt_pts, const int32_t *jobs4, const float *guesses9, int n_jobs, float *T_out9,
                               int32_t *status, int32_t *iters);
/* The outlier filters and transformation checker of a chain that sfe_icp_params has no field for (all zero: none of
 * them).  d2 is the matcher's float squared distance; a pair is kept only if every listed filter keeps it:
 *   MinDistOutlierFilter     d2 >= minDist * minDist (the square in float)
 *   MedianDistOutlierFilter  d2 <= factor * median (a float product), median = the (unsigned)(n * 0.5f)-th smallest (0-based)
 *                            of the n finite d2 -- the trimmed filter's quantile; none finite: SFE_ICP_NO_OUTLIER
 * BoundTransformationChecker on the accumulated T_iter (reference-mean frame, identity at the start): out of bounds when
 * acosf(T00) > max_rotation_norm (a NaN never is) or sqrtf(tx*tx + ty*ty) > max_translation_norm; the job then reports
 * SFE_ICP_BOUND with T = the guess.  The checkers run in the listed order: Bound is skipped on the iteration at which a
 * Counter listed before it reaches its limit (bound_order bit 0), and a Differential NaN status wins over Bound's only
 * when the Differential checker is listed first (bit 1). */
typedef struct sfe_icp_outliers {
    int use_min_dist;           /* MinDistOutlierFilter listed */
    float min_dist;             /*   .minDist (>= 0) */
    int use_median;             /* MedianDistOutlierFilter listed */
    float median_factor;        /*   .factor (finite, > 0) */
    int use_bound;              /* BoundTransformationChecker listed */
    float max_rotation_norm;    /*   .maxRotationNorm (finite, > 0) */
    float max_translation_norm; /*   .maxTranslationNorm (finite, > 0) */
    int bound_order;            /*   bit 0: CounterTransformationChecker listed before it, bit 1: Differential* listed before it */
} sfe_icp_outliers;
/* The *_chain entry points with those settings too; o == NULL is exactly the *_chain call. */
int sfe_icp_compute_guesses_chain_ext(sfe_ctx *ctx, const sfe_icp_params *p, const sfe_icp_outliers *o,
                                      const sfe_icp_dpf *rd, int n_rd, const sfe_icp_dpf *rf, int n_rf, const float *src,
                                      int n_src, const float *tgt, int n_tgt, const float *guesses9, int n_guesses,
                                      float *T_out9, int32_t *status, int32_t *iters);
int sfe_icp_compute_pairs_chain_ext(sfe_ctx *ctx, const sfe_icp_params *p, const sfe_icp_outliers *o,
                                    const sfe_icp_dpf *rd, int n_rd, const sfe_icp_dpf *rf, int n_rf, const float *src,
                                    const int32_t *src_off, const float *tgt, const int32_t *tgt_off, const float *guesses9,
                                    int n_jobs, float *T_out9, int32_t *status, int32_t *iters);
int sfe_icp_compute_jobs_chain_ext(sfe_ctx *ctx, const sfe_icp_params *p, const sfe_icp_outliers *o,
                                   const sfe_icp_dpf *rd, int n_rd, const sfe_icp_dpf *rf, int n_rf, const float *src,
                                   int n_src_pts, const float *tgt, int n_tgt_pts, const int32_t *jobs4, const float *guesses9,
                                   int n_jobs, float *T_out9, int32_t *status, int32_t *iters);
/* ---- the same chains on N x 3 clouds (a chain written for 3-D: icp_config.IcpChain with dims = 3) ----
 * Restated from libpointmatcher's published behaviour (parity unpinned, like the 2-D chain); each rule is the 2-D one with
 * one more coordinate.  Data-point stages are sfe_icp_dpf with the SFE_DPF_* kinds; a stage keeps a point (x, y, z) when
 *   SFE_DPF_MAX_DIST     dim -1: sqrtf(fl(fl(fl(x x) + fl(y y)) + fl(z z))) < |f[0]|; dim 0 / 1 / 2: x / y / z < f[0]
 *   SFE_DPF_MIN_DIST     dim -1: the same norm > |f[0]|; dim 0 / 1 / 2: |x| / |y| / |z| > |f[0]|
 *   SFE_DPF_BOUNDING_BOX (xMin < x < xMax && yMin < y < yMax && zMin < z < zMax) != remove_inside, f = xMin xMax yMin yMax
 *                        zMin zMax (all six are used)
 *   SFE_DPF_OCTREE_GRID  exactly sfe_downsample3(cloud, f[0]): the 8-way tree with its key and medoid rules and its leaf
 *                        order, bit for bit; the tree is cut at 21 levels like sfe_downsample3's, so no cloud is refused and
 *                        SFE_ICP_DPF_DEPTH never occurs in 3-D
 * Every product / sum is rounded to float, sqrtf is correctly rounded, the comparisons are strict: a NaN coordinate fails
 * them.  Kept points keep their order.  A cloud with z = 0 under a MAX_DIST / MIN_DIST stage with dim <= 1 keeps exactly
 * the points the 2-D stage keeps of its (x, y) columns.
 *
 * sfe_icp3_filter_clouds_dev runs n_stages stages in order over n_clouds device-resident clouds of packed float triples,
 * cloud c = d_pts[off[c] .. off[c+1]) (off: host, n_clouds + 1 entries, in points, each cloud <= 2^28 points).  The
 * survivors go to d_out back to back (cloud c after the survivors of clouds 0 .. c-1; d_out holds off[n_clouds] points
 * and does not overlap d_pts), their number to counts_out[c] (host).  Consecutive predicate stages are one pass; an
 * octree stage is one launch per step for all clouds.  One stream synchronisation, for the counts.  SFE_ERR_ARG before any
 * launch: a stage with dim > 2 or < -1, an octree size that is not finite and > 0, an unknown kind, more than
 * SFE_DPF_MAX_STAGES stages. */
int sfe_icp3_filter_clouds_dev(sfe_ctx *ctx, const sfe_icp_dpf *stages, int n_stages, const float *d_pts,
                               const int64_t *off, int n_clouds, float *d_out, int32_t *counts_out);
/* sfe_icp3_compute_jobs with a whole chain.  The reading stages run once on every distinct source slice of the call, the
 * reference stages once on every distinct target slice, each in the cloud's own frame before any guess is applied; ICP
 * then runs on the filtered clouds: the reference mean is the filtered target's, whether the LDS tile is resident or
 * streamed is decided by the filtered target's size, and with minimizer == 2 or 3 the normals are taken once per distinct
 * filtered target.  A job whose filtered reading or reference is empty reports SFE_ICP_DPF_EMPTY with T = the guess and 0
 * iterations; the other jobs are unaffected.
 * The modules of sfe_icp_outliers run inside the loop, on the matcher's float d2 of sfe_icp3_compute_jobs:
 *   MinDist     d2 >= fl(minDist minDist)
 *   MedianDist  d2 <= fl(factor x median), median = the (unsigned)(n x 0.5f)-th smallest (0-based) of the n finite d2;
 *               none finite: SFE_ICP_NO_OUTLIER
 * A pair is kept only if every listed filter, MaxDist and Trimmed included, keeps it; no pair kept: SFE_ICP_NO_POINT.
 * BoundTransformationChecker runs on the accumulated T_iter (reference-mean frame, identity at the start), in fp64 from the
 * float entries like the 3-D Differential checker: the rotation is 2 atan2(|vec q|, |w|) of the rotation block's
 * quaternion against the identity's (Eigen's branch rule), the translation sqrt((tx tx + ty ty) + tz tz); out of bounds
 * when the rotation > (double)max_rotation_norm or the translation > (double)max_translation_norm (a NaN never is).  The
 * job then reports SFE_ICP_BOUND with T = the guess.  Its place among the checkers is the 2-D rule: Bound is skipped on
 * the iteration at which a Counter listed before it reaches its limit (bound_order bit 0), and a Differential NaN status
 * wins over Bound's only when the Differential checker is listed first (bit 1).
 * With o == NULL (or all zero) and no stages the call is sfe_icp3_compute_jobs, bit for bit; a chain without the modules
 * of sfe_icp_outliers runs the kernel of sfe_icp3_compute_jobs.  SFE_ERR_ARG before any launch: what
 * sfe_icp3_filter_clouds_dev refuses in a stage list, and the outlier settings the 2-D *_chain_ext calls refuse. */
int sfe_icp3_compute_jobs_chain_ext(sfe_ctx *ctx, const sfe_icp_params *p, const sfe_icp_outliers *o, const sfe_icp_dpf *rd,
                                    int n_rd, const sfe_icp_dpf *rf, int n_rf, const float *src, int n_src_pts,
                                    const float *tgt, int n_tgt_pts, const int32_t *jobs4, const float *guesses16, int n_jobs,
                                    float *T_out16, int32_t *status, int32_t *iters);
/* A-B knob for the ICP kernels.  bit 2: 0 = strip-sweep exact NN search (default; targets beyond 8192
 * points are walked through L2 instead of LDS), 1 = brute-force tile scan for everything.
 * Brute-force only: bit 0: 0 = packed fp32 NN loop, 1 = scalar fp32; bit 1: 0 = 64-VGPR build,
 * 2 workgroups/CU, 1 = 128-VGPR build.  bit 3 (strip sweep only): the clouds and guesses handed to the ICP
 * entry points are final, i.e. no work enqueued earlier on this context still writes them; the preparation of
 * the targets (sort, strip table, normals) is then enqueued on a side stream of the lowest priority, not behind
 * that earlier work, and only the iteration kernel waits for both.  What the preparation writes exists twice and
 * consecutive batches use the copies in turn, so the preparation of a batch waits for the iteration kernel of the
 * batch two back, not for the one right before it, and runs beside that one (batches with jobs shared
 * by several workgroups, bit 4, keep the wait for the batch before).  The bit may change between two calls without
 * a synchronisation.  Leave it clear when a preceding call on the context produces the clouds.
 * bit 4: never share one large job between several workgroups.  Sharing (jobs of >= 8192 queries on a target beyond
 * 8192 points, when the call holds nothing else and shares x jobs <= CUs) needs every share resident at the same
 * time, which only a device this context has to itself can promise; a share that waits 0.5 s for the others gives up
 * and the job reports SFE_ICP_SPLIT_TIMEOUT.  The host-pointer entry points (sfe_icp_compute*) then launch the call once
 * more without sharing, so their callers never see that status; callers of the enqueue-only *_dev entry points that
 * share the device set the bit themselves or repeat the call with it when they read status 6.
 * All variants return identical results. */
int sfe_icp_set_tuning(sfe_ctx *ctx, int variant);
/* profile mode of the strip-sweep ICP kernel: enable/disable, and read the 96 values of the last profiled launch
 * (buffer of 96 long long; batches of more jobs than CUs with LDS-resident targets only).  [80..84] are counted
 * over the WHOLE launch: [80] candidate distance evaluations by the lane-per-query tiers, [81] by the cooperative
 * tier, [82] witness evaluations, [83] lower-bound probes, [84] ICP iterations run (all jobs).  The rest are
 * per-phase cycle counters of workgroup 0, summed over iterations.  Cycles: [0] setup incl. the
 * query sort, [1] first search pass (own strip), [3] trimmed quantile, [4] reduction, [5] solve, [6] later
 * search passes, [7] cooperative tier, [8] finite/exact census.  Counts: [9] search rounds, [10] queries
 * handed to the cooperative tier, [11] queries handed to the second pass, [12] cooperative trips.
 * [16 + 2i], [17 + 2i]: search cycles and (cap bits << 32 | exact matches) of iteration i < 32. */
int sfe_icp_get_profile(sfe_ctx *ctx, int enable, long long *cycles16);
/* test hook: the kernel the launcher gave each job of the last ICP call on this context, and the CU count its tier
 * rules used.  route may be NULL with n_jobs == 0 (just n_cu); SFE_ERR_ARG if n_jobs differs from that call's job count. */
#define SFE_ICP_ROUTE_TINY 0    /* one wave per job, exhaustive search (clouds of a few hundred points) */
#define SFE_ICP_ROUTE_T0 1      /* strip sweep, one-wave workgroups (many small jobs in the call) */
#define SFE_ICP_ROUTE_T1 2      /* strip sweep, four-wave workgroups */
#define SFE_ICP_ROUTE_Q 3       /* strip sweep, 1024 threads, target and per-query results in LDS */
#define SFE_ICP_ROUTE_LDS 4     /* ... target in LDS, per-query results in HBM scratch */
#define SFE_ICP_ROUTE_GLB 5     /* ... target in HBM scratch */
#define SFE_ICP_ROUTE_SPLIT 6   /* ... the job shared by several workgroups */
#define SFE_ICP_ROUTE_BRUTE 7   /* brute-force tile scan (sfe_icp_set_tuning bit 2) */
int sfe_icp_last_routes(sfe_ctx *ctx, int32_t *route, int n_jobs, int32_t *n_cu);
/* independent jobs, device-resident: clouds concatenated, job j uses
 * src[src_off[j]..src_off[j+1]) and tgt[tgt_off[j]..tgt_off[j+1]) (offsets in points, host
 * arrays of n_jobs+1), guess d_guess9 + 9*j; outputs d_T9 (9 floats), d_status, d_iters per job */
int sfe_icp_batch_dev(sfe_ctx *ctx, const sfe_icp_params *p, const float *d_src,
                      const int32_t *src_off, const float *d_tgt, const int32_t *tgt_off,
                      const float *d_guess9, int n_jobs, float *d_T9, int32_t *d_status,
                      int32_t *d_iters);

/* the same with a job table: jobs4 (host, n_jobs x 4) = (src_start, n_src, tgt_start, n_tgt) in points into the resident
 * clouds, so that jobs may share clouds -- the <= 30 guesses of compute_icp_with_cov on one pair (slam.py:346-358), one
 * target matched against many sources; jobs naming the same target slice share its preparation */
int sfe_icp_jobs_dev(sfe_ctx *ctx, const sfe_icp_params *p, const float *d_src, const float *d_tgt,
                     const int32_t *jobs4, const float *d_guess9, int n_jobs, float *d_T9, int32_t *d_status,
                     int32_t *d_iters);

/* Device-resident tail of FeatureExtraction.callback (feature_extraction.py:241-249) for a batch:
 * pcl.downsample(points, resolution) then pcl.remove_outlier(points, radius, min_points) on the
 * float64 clouds sfe_extract_points_batch_dev left in HBM (d_pts [n_frames][cap][2], d_counts),
 * without a host round trip.  resolution <= 0 skips the downsample (:241), min_points <= 1 the
 * outlier filter (:245).  Output: float32 clouds d_out [n_frames][cap][2] (what pybind hands back),
 * d_out_counts[f] points each (-1: the frame's octree is deeper than 24 levels).  cap <= 65536. */
int sfe_cloud_filter_batch_dev(sfe_ctx *ctx, const double *d_pts, const int32_t *d_counts, int n_frames,
                               int64_t cap, float resolution, double radius, int min_points,
                               float *d_out, int32_t *d_out_counts);
/* The same filters (feature_extraction.py:241-249; pcl.cpp:128-141, 54-74) on the clouds sfe_extract_points_bits_staged_dev
 * left staged on this context: same arguments minus the float64 points, same outputs, bit for bit (the float32 points are
 * those the cast of the call above produces; a bounding box does not depend on the order it is taken in). */
int sfe_cloud_filter_staged_dev(sfe_ctx *ctx, int n_frames, int64_t cap, float resolution, double radius,
                                int min_points, float *d_out, int32_t *d_out_counts);

/*
 * ONE ping through the whole of FeatureExtraction.callback (feature_extraction.py:223-249) in one call, for the live
 * node (one ping per callback: latency, not throughput): img (host, polar_rows x polar_cols uint8) goes up once through
 * pinned staging; CFAR + gate (alg / train_hs / guard_hs / k / tau / intensity_thr as for sfe_cfar_u8), remap +
 * nonzero + px->m, pcl.downsample(resolution) and pcl.remove_outlier(radius, min_points) run back to back on the
 * stream (resolution <= 0 / min_points <= 1 skip a filter like :241 / :245); the float32 cloud comes down once:
 * one stream synchronisation per ping.  cloud_out: host [cap x 2] float32 (y_forward, x_lateral), *n_out points;
 * *n_raw_out (nullable) = points before the filters.  vis_out (nullable, host cart_rows x cart_cols) additionally
 * receives cv2.remap(img) for the visualisation (:226).  Returns SFE_ERR_CAP when more than cap points were extracted
 * (*n_raw_out says how many: retry with a larger cap; cap <= 65536); *n_out = -1 when the cloud's octree is deeper
 * than the resident filter's 24 levels (take the per-cloud entry points).  Results are bit-identical to the chain of
 * sfe_cfar_u8 -> sfe_extract_points -> sfe_downsample -> sfe_remove_outlier.
 */
int sfe_feature_extract_ping(sfe_ctx *ctx, sfe_geom *g, const uint8_t *img, int alg, int train_hs, int guard_hs,
                             int k, double tau, int intensity_thr, float resolution, double radius, int min_points,
                             int64_t cap, float *cloud_out, int32_t *n_out, int32_t *n_raw_out, uint8_t *vis_out);

/* ---- device-resident keyframe clouds: the hand-off feature node -> SLAM node without PCIe ------------------
 * Reference flow (every cloud crosses the process boundary and is rebuilt in numpy):
 *   feature_extraction.py:175-193  publish_features           cloud -> PointCloud2 xyz32
 *   slam_ros.py:169-170            SLAM_callback              xyz -> [x, -z] (float64 array of float32 values:
 *                                                             ros_numpy pointcloud2_to_xyz_array)
 *   slam_objects.py:178-198        Keyframe.transform_points  points.dot(T[:2,:2].T) + T[:2,2], T float32
 *   slam.py:229-292                SLAM.get_points            transform, concatenate, pcl.downsample
 *   slam.py:294-323                SLAM.compute_icp           pcl.ICP.compute(source, target, guess)
 *   slam.py:389-424                SLAM.get_overlap           transform, pcl.match, count ids != -1
 * A store keeps the clouds in HBM: one pool of float2 points and a slot table (offset, count) per cloud.  A cloud is
 * named by its handle (slot index, handed out in order); slots are released in stack order (sfe_cloud_store_truncate):
 * keyframe clouds stay for the session, the target clouds get_points builds are dropped after their scan match.
 * Clouds are appended by kernels that read their sizes from device memory, so the sizes reach the host lazily: the
 * entry points that need them (meta, read, get_points, the scan match) copy the new slot-table entries down once
 * (a few bytes per cloud, one stream synchronisation) -- never the points.  A cloud's count is < 0 when its producer
 * failed: -1 the resident downsample refused it (octree deeper than 24 levels), -3 the pool was full. */
typedef struct sfe_cloud_store sfe_cloud_store;
#define SFE_STORE_NEGATE_Y 1   /* put: store (x, -y), what slam_ros.py:170 makes of the feature message */
#define SFE_PING_VIS_JET 4     /* sfe_feature_extract_ping_store: vis_out is the bgr8 image applyColorMap(remap(img), JET)
                                  (cart_rows x cart_cols x 3, feature_extraction.py:226-228) instead of the grey remap */
#define SFE_STORE_F32_POINTS 2 /* get_points / overlap: the caller's keyframe clouds are float32 numpy arrays (sgemm
                                  rounding: fma(p1, r1, p0 * r0) + t in float) instead of the SLAM node's float64 ones
                                  (products and sums in double, rounded to float32 at the pybind boundary) */
int sfe_cloud_store_create(sfe_ctx *ctx, int64_t capacity_points, int32_t max_clouds, sfe_cloud_store **out);
void sfe_cloud_store_destroy(sfe_cloud_store *s);
int sfe_cloud_store_count(sfe_cloud_store *s); /* slots in use = the next handle */
/* one cloud from the host (a feature message that arrived over the wire), enqueue only */
int sfe_cloud_store_put(sfe_ctx *ctx, sfe_cloud_store *s, int64_t stamp, const float *pts, int n, int32_t *handle_out);
/* ... with a key per point (keys[i] >= 0, else SFE_ERR_ARG and no slot): a keyed slot like the one
 * sfe_cloud_store_get_points_keys leaves, read back by sfe_cloud_store_read_keys.  For a cloud that arrives already keyed: the
 * SLAM cloud (x, y, 0, key) of slam_ros.py:317-359 as the mapping node receives it.  Enqueue only. */
int sfe_cloud_store_put_keys(sfe_ctx *ctx, sfe_cloud_store *s, int64_t stamp, const float *pts, const int32_t *keys, int n,
                             int32_t *handle_out);
/* n_frames clouds straight from sfe_cloud_filter_batch_dev's outputs (d_clouds [n_frames][cap][2] float32, d_counts),
 * device to device, enqueue only; stamps (host, nullable) are kept with the slots; handles_out (host, nullable) */
int sfe_cloud_store_put_batch_dev(sfe_ctx *ctx, sfe_cloud_store *s, const int64_t *stamps, const float *d_clouds,
                                  const int32_t *d_counts, int n_frames, int64_t cap, int flags, int32_t *handles_out);
/* slot table of clouds first .. first + n - 1 (each output nullable); synchronises if entries are new */
int sfe_cloud_store_meta(sfe_ctx *ctx, sfe_cloud_store *s, int32_t first, int32_t n, int64_t *stamps, int64_t *offsets,
                         int32_t *counts);
/* the points of one cloud, for whoever needs them on the host (the PointCloud2 of publish_features, rviz, mapping) */
int sfe_cloud_store_read(sfe_ctx *ctx, sfe_cloud_store *s, int32_t handle, float *out, int cap, int *n_out);
/* the points of n clouds back to back in `out` (room for cap points): one copy per cloud, one synchronisation at the end (the
 * copies land in pageable memory, so the runtime may stage each of them); counts_out[i] as
 * sfe_cloud_store_read's n_out (<= 0: nothing written for that cloud) */
int sfe_cloud_store_read_many(sfe_ctx *ctx, sfe_cloud_store *s, const int32_t *handles, int n, float *out, long long cap,
                              int32_t *counts_out);
/* release every slot >= n_slots */
int sfe_cloud_store_truncate(sfe_ctx *ctx, sfe_cloud_store *s, int32_t n_slots);
/* SLAM.get_points(frames, ref_frame) for n_jobs target clouds at once (slam.py:229-292): job j takes the clouds
 * handles[j*m .. j*m+m) (-1 = unused), moves cloud k by T6[(j*m+k)*6 ..] = {T00 T01 T02 T10 T11 T12} of
 * ref_pose.between(pose).matrix().astype(float32) like Keyframe.transform_points, concatenates them in that order and
 * runs pcl.downsample(resolution) (resolution <= 0: no downsample); the results become new slots (handles_out, host).
 * Targets of up to 65 536 points run on the resident filters, all jobs of the call in one launch each; a call with a
 * larger one (the loop-closure target of a long session, slam.py:999) takes its jobs one by one through a path without
 * a size limit.  A cloud whose count is < 0 is refused (SFE_ERR_ARG). */
int sfe_cloud_store_get_points(sfe_ctx *ctx, sfe_cloud_store *s, const int32_t *handles, const float *T6, int n_jobs, int m,
                               float resolution, int flags, const int64_t *stamps, int32_t *handles_out);
/* SLAM.compute_icp over handles (slam.py:294-323): pairs = n_jobs x (source handle, target handle); otherwise like
 * sfe_icp_jobs_dev (device guesses / results, enqueue only once the sizes are known) and sfe_icp_compute_jobs (host
 * guesses / results, one synchronisation).  Empty or failed clouds are refused (SFE_ERR_ARG): the caller tests
 * ssm_min_points first like slam.py:745. */
int sfe_icp_store_jobs_dev(sfe_ctx *ctx, const sfe_icp_params *p, sfe_cloud_store *s, const int32_t *pairs,
                           const float *d_guess9, int n_jobs, float *d_T9, int32_t *d_status, int32_t *d_iters);
int sfe_icp_store_compute(sfe_ctx *ctx, const sfe_icp_params *p, sfe_cloud_store *s, const int32_t *pairs,
                          const float *guesses9, int n_jobs, float *T_out9, int32_t *status, int32_t *iters);
/* sfe_icp_store_compute with a whole chain: o (may be NULL) as in sfe_icp_compute_jobs_chain_ext, rd / rf the reading
 * / reference data-point filter stages.  The pairs are refused as sfe_icp_store_compute refuses them.  No stage: the
 * sfe_icp_store_compute call under o.  With stages they read the store's pool in place, every distinct handle of a side
 * filtered once per call; results as sfe_icp_compute_jobs_chain_ext's (statuses 7, 8 and 9 with T = the guess).  The
 * octree stage rewrites the staging slots of sfe_extract_points_bits_staged_dev. */
int sfe_icp_store_compute_chain_ext(sfe_ctx *ctx, const sfe_icp_params *p, const sfe_icp_outliers *o,
                                    const sfe_icp_dpf *rd, int n_rd, const sfe_icp_dpf *rf, int n_rf,
                                    sfe_cloud_store *s, const int32_t *pairs, const float *guesses9, int n_jobs,
                                    float *T_out9, int32_t *status, int32_t *iters);
/* SLAM.get_overlap (slam.py:389-424) for n_jobs (source, target) pairs: the source moved by T6[j*6 ..] (the estimated
 * pose's matrix as float32), pcl.match(target, source, 1, max_dist), counts_out[j] = matched points (host) */
int sfe_cloud_store_overlap(sfe_ctx *ctx, sfe_cloud_store *s, const int32_t *pairs, const float *T6, int n_jobs,
                            float max_dist, int flags, int32_t *counts_out);
/* ---- loop-closure search over the store: slam.py:839-1001 (initialize_nonsequential_scan_matching) ----
 * get_points(target_frames, None, return_keys=True) (slam.py:873 -> :229-292): m keyframe clouds, cloud k moved by
 * T6[k*6 ..] (its own pose's matrix as float32) and tagged with keys[k]; pcl.downsample(points, keys, resolution), the
 * descriptor overload (pcl.cpp:143-159): a leaf's medoid brings its key along.  No size limit (every keyframe older than
 * k - min_st_sep goes in).  One new slot; its keys stay on the device next to its points. */
int sfe_cloud_store_get_points_keys(sfe_ctx *ctx, sfe_cloud_store *s, const int32_t *handles, const float *T6,
                                    const int32_t *keys, int m, float resolution, int flags, int64_t stamp, int32_t *handle_out);
int sfe_cloud_store_read_keys(sfe_ctx *ctx, sfe_cloud_store *s, int32_t handle, int32_t *out, int cap, int *n_out);
/* The field-of-view gate (slam.py:875-899) on a keyed cloud: source frame f sees a point iff, moved by Tinv6[f*6 ..]
 * (pose.inverse().matrix() as float32, float32 arithmetic like numpy's), its range is < range_bound[f] and |bearing| <
 * bearing_bound[f]; a point is selected iff some frame sees it.  key_counts_out[k] (host, n_keys entries) = selected
 * points with key k -- np.unique(keys[sel], return_counts=True), slam.py:902; *n_selected_out their number.  The
 * selection stays on the device for sfe_cloud_store_compact_selected.  *n_ambiguous_out = points whose bearing lies
 * within float32 rounding of a bound (numpy's float32 arctan2 is not reproduced bit for bit): if it is not 0 the caller
 * evaluates the gate with numpy and hands the selection over with sfe_cloud_store_set_selection. */
int sfe_cloud_store_fov_select(sfe_ctx *ctx, sfe_cloud_store *s, int32_t handle, const float *Tinv6, const double *range_bound,
                               const double *bearing_bound, int n_frames, int n_keys, int32_t *key_counts_out,
                               int32_t *n_selected_out, int32_t *n_ambiguous_out);
int sfe_cloud_store_set_selection(sfe_ctx *ctx, sfe_cloud_store *s, int32_t handle, const uint8_t *sel, int n);
/* target_points[sel], target_keys[sel] (slam.py:898-899): a new slot, order kept, keys kept */
int sfe_cloud_store_compact_selected(sfe_ctx *ctx, sfe_cloud_store *s, int32_t handle, int64_t stamp, int32_t *handle_out);
/* get_overlap(source under T6, target, return_indices=True) + np.unique(target_keys[indices[indices != -1]],
 * return_counts=True) (slam.py:977-985): pcl.match's neighbour (nearest, lowest index among equals, within max_dist) of
 * every source point; key_counts_out[k] = matches whose target carries key k, *overlap_out their number */
int sfe_cloud_store_match_keys(sfe_ctx *ctx, sfe_cloud_store *s, int32_t source, const float *T6, int32_t target, float max_dist,
                               int flags, int n_keys, int32_t *key_counts_out, int32_t *overlap_out);
/* The four calls above for n_jobs clouds at once, one launch per stage (chained.SessionBatch runs the loop-closure search of
 * all its sessions in lock-step).  Job by job the results equal the single-job calls bit for bit -- those are the n = 1 case.
 *   get_points_keys_many: job j = handles / T6 / keys [job_off[j], job_off[j + 1]) (job_off[0] = 0), its own downsample,
 *     its own new slot handles_out[j] (stamps: n_jobs entries or NULL).
 *   fov_select_many: job j = keyed cloud handles[j] against frames [frame_off[j], frame_off[j + 1]) of Tinv6 / range_bound /
 *     bearing_bound; key_counts_out[j * n_keys ..], n_selected_out[j], n_ambiguous_out[j].  Every cloud keeps its own
 *     selection (sfe_cloud_store_set_selection replaces one of them).
 *   compact_selected_many: handles_out[j] = the selected points of handles[j] (stamps: n_jobs entries or NULL).
 *   match_keys_many: job j = sources[j] under T6[j * 6 ..] against the keyed targets[j]; key_counts_out[j * n_keys ..],
 *     overlap_out[j]. */
int sfe_cloud_store_get_points_keys_many(sfe_ctx *ctx, sfe_cloud_store *s, const int32_t *handles, const float *T6,
                                         const int32_t *keys, const int32_t *job_off, int n_jobs, float resolution, int flags,
                                         const int64_t *stamps, int32_t *handles_out);
int sfe_cloud_store_fov_select_many(sfe_ctx *ctx, sfe_cloud_store *s, const int32_t *handles, int n_jobs, const float *Tinv6,
                                    const double *range_bound, const double *bearing_bound, const int32_t *frame_off,
                                    int n_keys, int32_t *key_counts_out, int32_t *n_selected_out, int32_t *n_ambiguous_out);
int sfe_cloud_store_compact_selected_many(sfe_ctx *ctx, sfe_cloud_store *s, const int32_t *handles, int n_jobs,
                                          const int64_t *stamps, int32_t *handles_out);
int sfe_cloud_store_match_keys_many(sfe_ctx *ctx, sfe_cloud_store *s, const int32_t *sources, const float *T6,
                                    const int32_t *targets, int n_jobs, float max_dist, int flags, int n_keys,
                                    int32_t *key_counts_out, int32_t *overlap_out);
/* bounding boxes of n clouds: bbox_out[i*4 ..] = {min x, min y, max x, max y} (float32 min / max: what np.min / np.max
 * of the cloud give, slam.py:506-507) */
int sfe_cloud_store_bbox(sfe_ctx *ctx, sfe_cloud_store *s, const int32_t *handles, int n, float *bbox_out);

/* sfe_feature_extract_ping with the cloud left in the store instead of copied to the host: the
 * filtered cloud becomes a new slot (with SFE_STORE_NEGATE_Y in flags: as the SLAM node holds it), *handle_out its
 * handle, *n_out its size; cloud_out (nullable, host [cap x 2], (forward, lateral) as published) receives the points
 * only when the caller wants to publish them.  On SFE_ERR_CAP / *n_out = -1 no slot is kept (*handle_out = -1); a store
 * whose pool has no room for the cloud is SFE_ERR_CAP as well (the slot's own count is read back with the two sizes).
 * s may be NULL (then cloud_out is required and handle_out may be NULL): the same call without a store, for the flags
 * sfe_feature_extract_ping has no argument for (SFE_PING_VIS_JET). */
int sfe_feature_extract_ping_store(sfe_ctx *ctx, sfe_geom *g, sfe_cloud_store *s, int64_t stamp, const uint8_t *img, int alg,
                                   int train_hs, int guard_hs, int k, double tau, int intensity_thr, float resolution,
                                   double radius, int min_points, int64_t cap, int flags, int32_t *handle_out,
                                   int32_t *n_out, int32_t *n_raw_out, float *cloud_out, uint8_t *vis_out);

/* ---- device-resident keyframe clouds in 3-D (sfe_store3.hip) ------------------------------------------------------
 * The keyframe store for N x 3 float32 clouds (Keyframe.points3D, slam_objects.py:101-106; the reference re-transforms
 * every keyframe's 3-D cloud on the host at every graph update, Keyframe.transform_points_3D, :200-223).  One pool of
 * packed points float[n][3] (12-byte stride, as sfe_match3 takes them) in HBM and a slot table (stamp, offset, count) per
 * cloud; a cloud is named by its handle (slot index, handed out in order) and slots are released in stack order.  Clouds
 * are packed back to back: a slot begins where the one before it ends.  The slot table lives on the host: a cloud comes
 * from the host (its size is known) or from sfe_cloud_store3_get_points (which synchronises once for the sizes), so no
 * entry point has to wait for sizes and no cloud can fail to fit after the fact -- a call that may not fit returns
 * SFE_ERR_CAP before it changes anything: no slot, no count, the next handle as it was.  Sizes and offsets are 64-bit (a
 * pool may pass 2^31 points); one cloud or one concatenation holds at most 2^28 points.
 *
 * The transform rule (get_points, overlap) is Keyframe.transform_points_3D's numpy expression on float32 arrays,
 * points.dot(H[:3, :3].T) + H[:3, 3], as numpy evaluates it: per output coordinate i
 *     fl( fma(p2, Hi2, fma(p1, Hi1, fl(p0 * Hi0))) + Hi3 )
 * (the 3-term form of SFE_STORE_F32_POINTS).  H12 = rows 0..2 of the 4 x 4 float32 matrix, row-major, 12 floats.
 *
 *
 * Keyed clouds.  A slot may carry an int32 key >= 0 per point (the keyframe index a point of the SLAM cloud came from) and a
 * selection byte per point, in two pools parallel to the point pool and indexed by the same offsets.  The two pools are
 * allocated at the first keyed call (put_keys, get_points_keys), so a store that never uses keys costs what it costs
 * without them; if that allocation fails the call returns SFE_ERR_HIP and nothing has changed.  With them the store runs
 * the SLAM cloud (get_points_keys) and the candidate selection of the loop-closure search (fov_select, compact_selected,
 * match_keys: slam.py:873-902, :977-997) over handles.  Every call that takes jobs runs one launch per stage for all of
 * them (at most 65 535); every call that creates slots tests an upper bound of its result before it launches anything,
 * returns SFE_ERR_CAP with the store untouched otherwise, and places its results compactly after one synchronisation for
 * the sizes.  All counts are integers: no result depends on the order of the atomics.
 *
 * Not provided in 3-D: a device-to-device producer (clouds come in through put / put_keys), and the FrontEnd /
 * SessionBatch wiring of the 2-D store. */
typedef struct sfe_cloud_store3 sfe_cloud_store3;
int sfe_cloud_store3_create(sfe_ctx *ctx, int64_t capacity_points, int32_t max_clouds, sfe_cloud_store3 **out);
void sfe_cloud_store3_destroy(sfe_cloud_store3 *s);
int sfe_cloud_store3_count(sfe_cloud_store3 *s); /* slots in use = the next handle */
/* one cloud from the host (pts [n][3]; n == 0: an empty slot), enqueue only.  SFE_ERR_CAP, and nothing changes, if the pool
 * or the slot table has no room for it. */
int sfe_cloud_store3_put(sfe_ctx *ctx, sfe_cloud_store3 *s, int64_t stamp, const float *pts, int n, int32_t *handle_out);
/* slot table of clouds first .. first + n - 1 (each output nullable); never synchronises */
int sfe_cloud_store3_meta(sfe_ctx *ctx, sfe_cloud_store3 *s, int32_t first, int32_t n, int64_t *stamps, int64_t *offsets,
                          int32_t *counts);
/* the points of one cloud (out: room for cap points of 3 floats; SFE_ERR_CAP with *n_out set if it holds more) */
int sfe_cloud_store3_read(sfe_ctx *ctx, sfe_cloud_store3 *s, int32_t handle, float *out, int cap, int *n_out);
/* release every slot >= n_slots and the pool behind them */
int sfe_cloud_store3_truncate(sfe_ctx *ctx, sfe_cloud_store3 *s, int32_t n_slots);
/* SLAM.get_points on 3-D clouds for n_jobs targets at once: job j takes the clouds handles[j*m .. j*m+m) (-1 = unused),
 * moves cloud k by H12[(j*m+k)*12 ..], concatenates them in list order and runs the 3-D pcl.downsample(resolution) -- the
 * 8-way tree, key and medoid rules of sfe_downsample3, bit for bit; resolution <= 0: no downsample.  Each result becomes a
 * new slot (handles_out, host; stamps nullable); a job without points gives an empty slot.  Every stage is one launch for
 * all jobs of the call (at most 65 535).  One synchronisation, for the jobs' output sizes; the results are placed compactly:
 * the next slot starts right behind the downsampled cloud.  SFE_ERR_CAP, and nothing changes, if the call's upper bound --
 * the sum of its input counts, or its n_jobs slots -- does not fit. */
int sfe_cloud_store3_get_points(sfe_ctx *ctx, sfe_cloud_store3 *s, const int32_t *handles, const float *H12, int n_jobs, int m,
                                float resolution, const int64_t *stamps, int32_t *handles_out);
/* sfe_icp3_compute_jobs over handles: pairs = n_jobs x (source handle, target handle), guesses / results 16 floats per job.
 * The same kernel on the store's pool, no point copied: T, status and iterations are bit for bit those of the host-pointer
 * call on the same clouds.  The same parameter check (minimizer 0, 2 or 3; with 2 or 3, pairs on one target handle share its
 * normals).  A pair that names an empty or unknown cloud is
 * refused with SFE_ERR_ARG before any launch. */
int sfe_icp3_store_compute(sfe_ctx *ctx, const sfe_icp_params *p, sfe_cloud_store3 *s, const int32_t *pairs,
                           const float *guesses16, int n_jobs, float *T_out16, int32_t *status, int32_t *iters);
/* ... with a whole chain: sfe_icp3_compute_jobs_chain_ext over handles, bit for bit.  The filtered clouds go to context
 * scratch; the store's slots, pool and count are unchanged afterwards.  o == NULL and no stages: sfe_icp3_store_compute. */
int sfe_icp3_store_compute_chain_ext(sfe_ctx *ctx, const sfe_icp_params *p, const sfe_icp_outliers *o, const sfe_icp_dpf *rd,
                                     int n_rd, const sfe_icp_dpf *rf, int n_rf, sfe_cloud_store3 *s, const int32_t *pairs,
                                     const float *guesses16, int n_jobs, float *T_out16, int32_t *status, int32_t *iters);
/* SLAM.get_overlap in 3-D for n_jobs (source, target) pairs in one launch: the source moved by H12[j*12 ..];
 * counts_out[j] = its points with a target point within max_dist under the rules of sfe_match3: d2 =
 * fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)), matched iff d2 <= fl(max_dist * max_dist), NaN and infinite distances never.
 * An empty source or target counts 0; an unknown handle is SFE_ERR_ARG. */
int sfe_cloud_store3_overlap(sfe_ctx *ctx, sfe_cloud_store3 *s, const int32_t *pairs, const float *H12, int n_jobs,
                             float max_dist, int32_t *counts_out);
/* sfe_cloud_store3_put with a key per point: a keyed slot from the host.  Any keys[i] < 0 is SFE_ERR_ARG and leaves no slot;
 * n == 0 gives an empty keyed slot. */
int sfe_cloud_store3_put_keys(sfe_ctx *ctx, sfe_cloud_store3 *s, int64_t stamp, const float *pts, const int32_t *keys, int n,
                              int32_t *handle_out);
/* 1: the slot carries keys; 0: it does not; SFE_ERR_ARG: no such slot (or s == NULL) */
int sfe_cloud_store3_keyed(sfe_cloud_store3 *s, int32_t handle);
/* SLAM.get_points(frames, ref, return_keys=True) on 3-D clouds (slam.py:229-292; the SLAM cloud of slam_ros.py:317-359) for
 * n_jobs targets at once.  Job j takes the entries [job_off[j], job_off[j+1]) of handles / H12 (12 floats each) / keys
 * (job_off[0] == 0; a handle of -1 is unused).  Cloud k is moved by H12[k*12 ..] under the store's transform rule, every one
 * of its points is tagged keys[k] (>= 0, else SFE_ERR_ARG), and the clouds are concatenated in list order.  The job then
 * runs the 3-D pcl.downsample(points, keys, resolution), the descriptor overload: the points are those of
 * sfe_cloud_store3_get_points for the same inputs, and a leaf's medoid brings its tag along.  resolution <= 0: the tagged
 * concatenation itself.  Inputs may be plain or keyed slots; a stored key is ignored.  Each result is one new keyed slot.
 * Launches, synchronisation, placement and SFE_ERR_CAP as in sfe_cloud_store3_get_points. */
int sfe_cloud_store3_get_points_keys(sfe_ctx *ctx, sfe_cloud_store3 *s, const int32_t *handles, const float *H12,
                                     const int32_t *keys, const int32_t *job_off, int n_jobs, float resolution,
                                     const int64_t *stamps, int32_t *handles_out);
/* the keys of one keyed cloud (out: room for cap keys; SFE_ERR_CAP with *n_out set if it holds more).  A plain slot is
 * SFE_ERR_ARG. */
int sfe_cloud_store3_read_keys(sfe_ctx *ctx, sfe_cloud_store3 *s, int32_t handle, int32_t *out, int cap, int *n_out);
/* The field-of-view gate of the loop-closure search (slam.py:875-899) with one more coordinate in the transform and the
 * range, for n_jobs keyed clouds in one launch: job j = cloud handles[j] against frames [frame_off[j], frame_off[j+1])
 * (frame_off[0] == 0) of Hinv12 (12 floats per frame: rows 0..2 of pose.inverse()) / range_bound / bearing_bound.  For point
 * p and frame f, q = p moved by Hinv12[f] (the store's transform rule),
 *     range = sqrtf(fl(fl(fl(qx qx) + fl(qy qy)) + fl(qz qz)))       correctly rounded: np.linalg.norm(local, axis=1) on
 *                                                                    a float32 N x 3 array
 * and f sees p iff (double)range < range_bound[f] and |atan2(qy, qx)| < bearing_bound[f].  The bearing is the horizontal
 * one, over the x and y columns, as mapping.py:183-185 takes it from 3-column points; there is no elevation gate because the
 * reference has none, so a z = 0 cloud gives the 2-D gate's result.  A point is selected iff some frame sees it.
 * key_counts_out[j*n_keys + k] = the selected points of job j with key k (keys >= n_keys are selected but not counted);
 * n_selected_out[j], n_ambiguous_out[j] per job.  The ambiguity rule is sfe_cloud_store_fov_select's: atan2 runs in double
 * and decides only outside 1e-6 a + 1e-30 of the bound; a point that no frame selects for certain and some frame leaves
 * undecided counts as ambiguous and is left unselected -- the caller then evaluates the gate in numpy for that cloud and
 * hands the result to sfe_cloud_store3_set_selection.  The selection bytes stay on the device, per cloud (a cloud named
 * by two jobs of one call keeps the bytes of one of them).  A plain slot is SFE_ERR_ARG. */
int sfe_cloud_store3_fov_select(sfe_ctx *ctx, sfe_cloud_store3 *s, const int32_t *handles, int n_jobs, const float *Hinv12,
                                const double *range_bound, const double *bearing_bound, const int32_t *frame_off, int n_keys,
                                int32_t *key_counts_out, int32_t *n_selected_out, int32_t *n_ambiguous_out);
/* the host's selection (a byte per point, non-zero = selected) replaces the device's; n must equal the cloud's count */
int sfe_cloud_store3_set_selection(sfe_ctx *ctx, sfe_cloud_store3 *s, int32_t handle, const uint8_t *sel, int n);
/* points[sel], keys[sel] (slam.py:898-899) of n_jobs keyed clouds, order kept: each result is a new keyed slot (empty if
 * nothing was selected).  A cloud for which no selection was written (by fov_select or set_selection) is SFE_ERR_ARG.
 * SFE_ERR_CAP, and nothing changes, if the call's upper bound -- the sum of its clouds' counts, or its n_jobs slots --
 * does not fit. */
int sfe_cloud_store3_compact_selected(sfe_ctx *ctx, sfe_cloud_store3 *s, const int32_t *handles, int n_jobs,
                                      const int64_t *stamps, int32_t *handles_out);
/* get_overlap(..., return_indices=True) and the per-key count of slam.py:977-985 for n_jobs pairs in one launch: job j
 * moves source pairs[2j] by H12[j*12 ..]; every moved point gets its sfe_match3 neighbour in the keyed target pairs[2j+1]
 * (the nearest point, the lowest index among equal distances, kept iff d2 <= fl(max_dist * max_dist); NaN and infinite
 * distances never match).  key_counts_out[j*n_keys + k] = the matches whose neighbour has key k (keys >= n_keys are not
 * counted); overlap_out[j] = the number of matches = what sfe_cloud_store3_overlap returns for the pair.  An empty source
 * or target gives zeros; a plain target is SFE_ERR_ARG. */
int sfe_cloud_store3_match_keys(sfe_ctx *ctx, sfe_cloud_store3 *s, const int32_t *pairs, const float *H12, int n_jobs,
                                float max_dist, int n_keys, int32_t *key_counts_out, int32_t *overlap_out);

/* ---- global-initialisation matching cost: slam.py:461-570 ---------------- */
/*
 * get_matching_cost_subroutine1 builds a dilated occupancy grid of the target cloud and hands
 * scipy.optimize.shgo a function that counts the source points falling on set cells under a
 * candidate transform (slam.py:692-701, 952-961 call it 50-500+ times per keyframe, one pose per
 * call).  Here the grid lives on the device and MANY candidate transforms are scored per launch.
 *
 * sfe_costgrid_create: tgt_r / tgt_c = the target cells exactly as slam.py:515-518 computes them
 * (rounded, clipped; host int32), rows x cols = target_grids.shape, dilate_hs = slam.py:522.  The
 * grid is target_grids after cv2.dilate with getStructuringElement(MORPH_ELLIPSE, (2h+1, 2h+1), (h, h)).
 */
typedef struct sfe_costgrid sfe_costgrid;
int sfe_costgrid_create(sfe_ctx *ctx, const int32_t *tgt_r, const int32_t *tgt_c, int n_tgt, int rows,
                        int cols, int dilate_hs, sfe_costgrid **out);
/* The same for n device-resident target clouds at once (one grid each, e.g. one per session): grid i is built from
 * cloud target_handles[i] of the store with the cells of slam.py:514-517 computed on the device in the cloud's dtype
 * (float32: (p - min) / float32(resolution), half to even, clipped); xmin / ymin / rows / cols [n] are what the
 * caller's numpy made of the cloud's bounding box (slam.py:506-511; sfe_cloud_store_bbox brings the box).  Enqueue only. */
int sfe_costgrid_create_store(sfe_ctx *ctx, sfe_cloud_store *s, const int32_t *target_handles, int n, const float *xmin,
                              const float *ymin, float resolution, const int32_t *rows, const int32_t *cols, int dilate_hs,
                              sfe_costgrid **out);
void sfe_costgrid_destroy(sfe_costgrid *g);
/* dilated grid `index` as the reference holds it: rows x cols uint8, 0 / 255 (host buffer) */
int sfe_costgrid_download(sfe_ctx *ctx, sfe_costgrid *g, int index, uint8_t *grid_out);
/*
 * The body of `subroutine` (slam.py:531-564) for n_poses transforms.  src: n_src x 2 float32 source
 * points (host); T6: per pose the float32 entries T00 T01 T02 T10 T11 T12 of
 * sample_transform.matrix(); xmin, ymin (float32, slam.py:506), resolution (slam.py:508);
 * cost_out[p] = -(number of source points on a set cell).
 * flags & SFE_COST_F64_POINTS: the source cloud is a float64 numpy array of float32 values (the SLAM node's keyframe
 * clouds, slam_ros.py:169-170): moved point and cell in double, as numpy promotes them; otherwise a float32 cloud (what
 * get_points returns: sgemm arithmetic, cell in float32 with float32(resolution)).
 */
#define SFE_COST_F64_POINTS 1
int sfe_matching_cost_batch(sfe_ctx *ctx, sfe_costgrid *g, const float *src, int n_src, const float *T6,
                            int n_poses, float xmin, float ymin, double resolution, int flags, int32_t *cost_out);
/* ... over store handles, n_jobs (source cloud, grid) pairs in one launch: job i scores source cloud source_handles[i]
 * against grid grid_index[i] of `g` (NULL: grid i, n_jobs = the number of grids) under the transforms
 * T6[(i * n_poses + p) * 6 ..]; cost_out[i * n_poses + p] (host).  One synchronisation. */
int sfe_matching_cost_store(sfe_ctx *ctx, sfe_costgrid *g, sfe_cloud_store *s, const int32_t *source_handles,
                            const int32_t *grid_index, int n_jobs, const float *T6, int n_poses, double resolution, int flags,
                            int32_t *cost_out);

/* ... the sample transforms computed on the device: job i scores source_handles[i] against its grid under
 * target_i.between(source_i.compose(delta_j)).matrix() (slam.py:548-550) for n_deltas deltas shared by all jobs; poses as
 * {x, y, cos(theta), sin(theta)} doubles (host): target_xycs / source_xycs [n_jobs x 4], delta_xycs [n_deltas x 4];
 * cost_out[i * n_deltas + j].  gtsam.Pose2's double arithmetic as sfe_pose2_sample_transforms below, bit for bit. */
int sfe_matching_cost_store_samples(sfe_ctx *ctx, sfe_costgrid *g, sfe_cloud_store *s, const int32_t *source_handles,
                                    const int32_t *grid_index, int n_jobs, const double *target_xycs, const double *source_xycs,
                                    const double *delta_xycs, int n_deltas, double resolution, int flags, int32_t *cost_out);

/* ---- replaces: everything scipy.optimize.shgo(func, bounds, n, iters=1, sampling_method="sobol", minimizer_kwargs=
 * {"options": {"ftol": ...}}) of slam.py:692-701 does AFTER its sampling stage, for n_problems cost tables at once (host only,
 * no device work).  Holds for the piecewise-constant cost of slam.py:529-567 only.  The vertex graph (CSR nn_off / nn_idx over
 * n_vertices vertices in shgo's vertex-cache order), the vertices x [n_vertices x 3] and the three forward-difference points of
 * SLSQP per vertex come from one run of the installed scipy (sonar_slam_amd/shgo_fast.py, SobolPlan);
 * tables [n_problems x n_vertices x 4]: the cost at each vertex and at its three finite-difference points.
 * status_out: SFE_SHGO_OK (result = vertex_out), SFE_SHGO_OK_TIED (several local results share the lowest cost: the caller asks
 * np.argsort over the costs of order_out[.. n_order_out], as shgo does -- its sort kernel is not stable), SFE_SHGO_FAILED (no
 * vertex strictly below all its neighbours: shgo's success = False, vertex_out = the lowest vertex), SFE_SHGO_FALLBACK (a
 * finite-difference point costs something else than its vertex or more than SFE_SHGO_MAX_POOL minimisers: run
 * scipy.optimize.shgo itself; two pool members equally far from the last result: the order is numpy's sort kernel's choice,
 * shgo_fast.py asks it).  order_out [n_problems x SFE_SHGO_MAX_POOL]: the
 * vertices in the order shgo minimises them. */
#define SFE_SHGO_OK 0
#define SFE_SHGO_FAILED 1
#define SFE_SHGO_FALLBACK 2
#define SFE_SHGO_OK_TIED 3
#define SFE_SHGO_MAX_POOL 32
int sfe_shgo_sobol_replay(int n_vertices, const int32_t *nn_off, const int32_t *nn_idx, const double *x, const int32_t *tables,
                          int n_problems, uint8_t *status_out, int32_t *vertex_out, int32_t *n_order_out, int32_t *order_out);
/* T6_out[(i * n_deltas + j) * 6 ..] = float32 rows of target_i.between(source_i.compose(delta_j)).matrix() (slam.py:548-550:
 * the sample transform of the matching cost) for n_sessions pose pairs x n_deltas deltas; every pose as {x, y, cos(theta),
 * sin(theta)} doubles.  gtsam.Pose2's expressions as sonar_slam_amd/pose2.py states them, in double, in the same order.  Host only. */
int sfe_pose2_sample_transforms(const double *target_xycs, const double *source_xycs, int n_sessions, const double *delta_xycs,
                                int n_deltas, float *T6_out);

/* ---- replaces: the log-odds occupancy grid of bruce_slam/mapping.py (method 1: add_keyframe, update_pose, fit_grid,
 * inc_grid / dec_grid, adjust_bounds, get_occupancy_grid1); sonar_slam_amd/mapping.py is the host side.  One sfe_map per
 * Mapping owns the device state: the float32 grid [rows x cols], the sonar_xy table of every geometry, and per keyframe slot
 * its polar log-odds image and its current cell list (r, c, l in ascending r * cols + c).  Entry points take host pointers.
 * An sfe_map is a one-map sfe_mapset, described below, and every call here is the sfe_mapset call of the same name over map 0.
 * What differs is where the slots live: an sfe_map has no arena and so no cap on slots or pixels (beyond the 2^30 pixels of
 * an image): a slot's buffers are allocated at its geometry's pixel count when its measurement (or sfe_map_set_logodds) runs.
 *   sfe_map_geometry: sonar_xy [img_rows * img_cols][2] float32 (mapping.py:158-163) -> geometry id.
 *   sfe_map_set_logodds: a ready log-odds image [img_rows * img_cols] for `slot` (created for `geom` on first use).
 *   sfe_map_measure: n keyframes at once: slot / geometry, hits [2 * hit_off[n]] (row, col of the downsampled image; keyframe b
 *     owns [hit_off[b], hit_off[b + 1])), hrhc[2 b] = hr, hc (hr < 0: no points, all miss_prob), its float32 kernel
 *     (2 hr + 1) x (2 hc + 1) at ktab + k_off[b], div[b] = kernel[hr, hc] / hit_prob; logit of miss32 / hit32 as the host
 *     computes it.  sfe_map_measure_stages reads keyframe b of the last call: hit mask, the image before logit, first hits.
 *   sfe_map_fit_bounds: per keyframe {min r, max r, min c, max c} of its pixels fitted with pose4 = {cos, sin, x, y} at
 *     origin2 = {y0, x0} (one synchronisation).
 *   sfe_map_grow: pad the grid by rows on top / bottom and columns left / right (existing cells keep their values).
 *   sfe_map_refit: fit, deduplicate (first pixel per cell) and apply n keyframes in order: for each, subtract its current
 *     list if dec[b], then add the new one.  mm = the bounds sfe_map_fit_bounds gave at the same origin, shift2 = {rows,
 *     cols} added to the fitted cells to reach the grid's current coordinates.  Enqueue only; a slot at most once per call.
 *   sfe_map_cells / sfe_map_logodds / sfe_map_read_grid: read back (which = 1: the grid of the last sfe_map_frames call);
 *     sfe_map_shape -> {rows, cols, rows grown on top, columns grown on the left}.
 *   sfe_map_frames: a fresh grid, the listed slots added in list order.  sfe_map_render: rows r0..r1 x cols c0..c1 of a grid
 *     -> int8(clip(100 expit(v), 0, 100)), resized INTER_NEAREST to out_h x out_w with source index floor(i * inv) when
 *     resize != 0.  sfe_map_render2: sfe_mapset_render2, below, for one image of this map; sfe_map_render2_store:
 *     sfe_mapset_render2_store for one image, its frame list frames[0 .. n_frames).
 *   sfe_map_hit_table / sfe_map_measure_store / sfe_map_measure_store_undecided / sfe_map_measure_store_finish: the store
 *     feed of one map: the sfe_mapset_* calls of the same names, below, over one map.  n keyframes of the map per call, each
 *     slot at most once.  A slot that holds an image of another geometry, an unknown geometry or a negative slot is refused
 *     with SFE_ERR_ARG, as by sfe_map_measure; a slot gets its storage only when its measurement runs, so a refused or
 *     dropped call leaves none behind (a measurement that fails with SFE_ERR_HIP leaves the slot unused, its buffers kept
 *     for the next call that names it).
 *   As the set's calls, sfe_map_fit_bounds, sfe_map_refit and sfe_map_measure_store take at most 65535 keyframes per call. */
typedef struct sfe_map sfe_map;
int sfe_map_create(sfe_ctx *ctx, int rows, int cols, sfe_map **out);
void sfe_map_destroy(sfe_map *m);
int sfe_map_geometry(sfe_map *m, const float *sonar_xy, int img_rows, int img_cols, int *id_out);
int sfe_map_set_logodds(sfe_map *m, int slot, int geom, const float *logodds);
int sfe_map_measure(sfe_map *m, int n, const int32_t *slots, const int32_t *geoms, const int32_t *hit_off,
                    const int32_t *hits, const int32_t *hrhc, const int32_t *k_off, const float *ktab, int n_ktab,
                    const double *div, float miss32, float logit_miss, float hit32, float logit_hit);
int sfe_map_measure_stages(sfe_map *m, int b, uint8_t *hits_out, float *prob_out, int32_t *first_hits_out);
int sfe_map_hit_table(sfe_map *m, const float *bearings, int num_bearings, const double *breaks, const double *coef,
                      int n_intervals, double margin, int num_ranges, double range_resolution, int range_in_double, int r_skip,
                      int c_skip, int *id_out);
int sfe_map_measure_store(sfe_map *m, sfe_cloud_store *store, int n, const int32_t *slots, const int32_t *geoms,
                          const int32_t *handles, const int32_t *tabs, double radius, int min_points, const int32_t *hrhc,
                          const int32_t *k_off, const float *ktab, int n_ktab, const double *div, float miss32,
                          float logit_miss, float hit32, float logit_hit, int32_t *n_points_out, int32_t *n_undecided_out);
int sfe_map_measure_store_undecided(sfe_map *m, float *xy_out, int32_t *pos_out, int cap);
int sfe_map_measure_store_finish(sfe_map *m, int n_cells, const int32_t *pos, const int32_t *cells);
int sfe_map_fit_bounds(sfe_map *m, int n, const int32_t *slots, const double *pose4, const double *origin2,
                       double resolution, int32_t *mm_out);
int sfe_map_grow(sfe_map *m, int top, int bottom, int left, int right);
int sfe_map_refit(sfe_map *m, int n, const int32_t *slots, const double *pose4, const double *origin2, double resolution,
                  const int32_t *mm, const int32_t *shift2, const uint8_t *dec);
int sfe_map_cells(sfe_map *m, int slot, uint16_t *r_out, uint16_t *c_out, float *l_out, int cap, int *n_out);
int sfe_map_logodds(sfe_map *m, int slot, float *out, int cap);
int sfe_map_shape(sfe_map *m, int32_t *rows_cols_grow4);
int sfe_map_read_grid(sfe_map *m, int which, float *out, long long cap);
int sfe_map_frames(sfe_map *m, int n, const int32_t *slots);
int sfe_map_render(sfe_map *m, int which, int r0, int r1, int c0, int c1, int out_h, int out_w, double inv, int resize,
                   int8_t *occ_out);
int sfe_map_render2(sfe_map *m, int n_slots, const int32_t *slots, int r0, int r1, int c0, int c1, const double *xy, int n_pts,
                    int filter, double radius, int min_points, int dilate_hs, double y0, double x0, double resolution,
                    int out_h, int out_w, double inv, int resize, int8_t *occ_out);
int sfe_map_render2_store(sfe_map *m, sfe_cloud_store *store, int n_slots, const int32_t *slots, int r0, int r1, int c0, int c1,
                          int handle, int all_frames, const int32_t *frames, int n_frames, int filter, double radius,
                          int min_points, int dilate_hs, double y0, double x0, double resolution, int out_h, int out_w,
                          double inv, int resize, int8_t *occ_out);

/* ---- S occupancy maps that advance together (sonar_slam_amd/mapping.py: MapBatch; chained.SessionBatch's maps).  One
 * sfe_mapset owns the state of n_maps maps, each exactly what an sfe_map of its own holds after the same calls: the
 * float32 grids (each with its own rows, columns and growth counters), one table of sonar_xy geometries shared by all maps,
 * and for every (map, slot) its polar log-odds image and its double-buffered cell list.  Every stage is one call over any
 * subset of the maps; a keyframe is named by (map, slot).  Entry points take host pointers.
 *
 * Memory: the arena is allocated once, at creation, for n_maps * max_keyframes slots of max_px pixels each and is never
 * reallocated: per keyframe max_px * 20 bytes (float32 log-odds 4 B, two cell lists of uint16 r + uint16 c + float32 l = 8 B
 * each, per pixel) + 8 bytes of counts; 2.1 MB at the 105 k pixels of a 1024 x 512 ping at the shipped skips.  A slot >=
 * max_keyframes or a geometry of more than max_px pixels is refused with SFE_ERR_CAP before anything changes.  Only this
 * arena is fixed.  Grids are reallocated when they grow, a frames grid when its map's shape changed, and the grow-only scratch
 * (job tables, measurement mask and image, render output, fit windows) when a call needs more than any before it, each with a
 * stream synchronisation.  The fit windows of one refit call lie back to back, 4 bytes per cell of every listed keyframe's
 * bounding box (about 360 KB for a 30 m fan at 0.2 m), and are kept: a caller with very many keyframes bounds that by the
 * number of keyframes it lists per call.
 *   sfe_mapset_create: every map starts as a zero grid [rows x cols].
 *   sfe_mapset_geometry: as sfe_map_geometry, for all maps (the caller stores equal tables once).
 *   sfe_mapset_set_logodds: n ready log-odds images, back to back in `logodds`, image b for (maps[b], slots[b]) of geometry
 *     geoms[b].  One synchronisation.
 *   sfe_mapset_measure: sfe_map_measure over (map, slot) jobs: all hits in one upload.  One synchronisation.
 *     sfe_mapset_measure_stages reads job b of the last call.
 *   sfe_mapset_measure_store: the same measurement with the hits taken on the device from clouds of a cloud store of the same
 *     context: job b = the cloud handles[b] for (maps[b], slots[b]) of geometry geoms[b], read with hit table tabs[b].
 *     Phase one, in this call: the radius outlier filter of every cloud (sfe_remove_outlier's decision; skipped for
 *     min_points <= 1), then per kept point its polar cell (row, column) / skips into the set's hit buffer -- the row
 *     exactly as numpy computes it for float32 points, the column from atan2 in double and the hit table's cubic, and only
 *     where that is safe (the guard band, below); every other point goes to its job's undecided list.  One read-back of n
 *     counters: n_points_out[b] = the cloud's size, n_undecided_out[b] = its undecided points.  If none is undecided the
 *     measurement runs at once and the call is complete; no point crosses to the host.  Otherwise the call is left pending:
 *     sfe_mapset_measure_store_undecided copies the undecided points out (xy_out[2 i ..], pos_out[i] = the point's entry
 *     in the hit buffer, ascending; cap >= their number), and phase two, sfe_mapset_measure_store_finish, takes the host's
 *     (row, column) for exactly those entries and runs the measurement.  Any later measure call drops a pending one, which
 *     has changed nothing.  hrhc / k_off / ktab / div are per job as in sfe_mapset_measure, given as for a cloud with points:
 *     a cloud of zero points becomes a keyframe without a measurement (hr < 0, all miss_prob), a cloud the filter empties
 *     keeps hr >= 0 with no hits.  Refused before anything changes: a handle the store does not hold or whose count is
 *     negative (a failed producer), an unknown table and a (map, slot) named twice in the call (a slot holds one image; checked
 *     after the per-job checks) with SFE_ERR_ARG, a slot >= max_keyframes with SFE_ERR_CAP (a
 *     geometry of more than max_px pixels is never registered: sfe_mapset_geometry refuses it with SFE_ERR_CAP).
 *   sfe_mapset_hit_table: what the cells need of a sonar geometry, stored once: the float32 bearings (their ends bound the
 *     table), oculus.b2c's cubic spline as n_intervals + 1 ascending knots and 4 double coefficients per interval (powers
 *     of (angle - knot), highest first), margin = 2 * ulp_float32(max(1, |bearing|)) * max(1, largest column slope) + 1e-9,
 *     num_ranges, range_resolution (range_in_double: the row in float64, for a numpy float64 scalar resolution) and the skips.
 *     Guard band: a point is decided only if its column value is further than margin from every x.5 and its angle further
 *     than margin from both ends of the table (outside the table the column is 0).
 *   sfe_mapset_fit_bounds: as sfe_map_fit_bounds; keyframe b carries its own pose and its own map's origin.  One synchronisation.
 *   sfe_mapset_grow: pad map maps[b] by grow4[4 b ..] = {top, bottom, left, right} (each map at most once per call); a map
 *     with four zeros costs nothing; one synchronisation for all the maps that grew.
 *   sfe_mapset_refit: fit and deduplicate all n keyframes in one pass (each keyframe's window is sized by its own bounds),
 *     then the ordered applies.  The keyframes of one map are applied in the order they are listed (subtract the current list
 *     if dec[b], then add the new one); maps are independent, so the i-th apply of every map runs in one launch: K refits per
 *     map cost 2 K launches (K without dec), however many maps take part.  Enqueue only; a (map, slot) at most once per call.
 *   sfe_mapset_cells / _logodds / _read_grid / _shape: read back one map's or one keyframe's state, as the sfe_map calls.
 *   sfe_mapset_apply_launches: the apply launches (rounds) the set has made since it was created, refit and frames alike.
 *   sfe_mapset_frames: for map maps[b] a fresh grid with slots[slot_off[b] .. slot_off[b + 1]) added in list order (rounds as
 *     in refit).  Enqueue only.
 *   sfe_mapset_render: n images in one launch and one read-back: job b renders box4[4 b ..] = {r0, r1, c0, c1} of map maps[b]'s
 *     grid (which[b] = 1: its frames grid) to out_hw[2 b ..] = {out_h, out_w} at occ_out + out_off[b]; `total` bytes in all.
 *     inv / resize as sfe_map_render.
 *   sfe_mapset_render2: the point-projection map (method 2: get_occupancy_grid2, mapping.py:357-439), n images in one call
 *     and one read-back; int8 cells of -1 (unknown), 0 (free) and 100 (occupied).  Job b works on the known region box4[4 b ..]
 *     = {r0, r1, c0, c1} of map maps[b] -- the caller's: the union of the boxes of the listed keyframes -- whose corner lies at
 *     origin2[2 b ..] = {y0, x0} metres: every cell of the current lists of slots[slot_off[b] .. slot_off[b + 1]) is free;
 *     its points are xy[2 pt_off[b] .. 2 pt_off[b + 1]) (float64 x, y; all jobs in one upload).  With filter[b] != 0 the
 *     points are rounded to float32 and go through sfe_remove_outlier's decision with radius[b] / min_points[b], and the kept
 *     float32 points are projected; otherwise the doubles are.  Projection: r = rint((y - y0) / resolution[b]), c likewise,
 *     in double; a point outside the region is dropped.  Every region cell under the element
 *     getStructuringElement(MORPH_ELLIPSE, (2 dilate_hs[b] + 1,) * 2) of a projected point becomes 100, above 0.  The region
 *     is then resized as in sfe_mapset_render (out_hw / inv / resize / out_off / total).  A region that is empty, leaves the
 *     map or lists a slot without cells is refused with SFE_ERR_ARG; at most 65535 jobs and 65535 listed slots per call.
 *   sfe_mapset_render2_store: sfe_mapset_render2 with job b's points taken in place from cloud handles[b] of `store` (a store
 *     of the set's context): no point and no key is copied, the image is the only read-back.  all_frames[b] != 0 takes every
 *     point of the cloud; otherwise the selection of mapping.py:365-372 over frames[frame_off[b] .. frame_off[b + 1]): for
 *     every listed k, the points whose key is k -- a key listed twice gives its points twice (they count twice in the filter),
 *     a k no point carries (a negative one, a key beyond the session) gives none, an empty list no point at all.  The stored
 *     float32 points go to the filter's decision as they are when filter[b] != 0, and the kept ones (all selected ones
 *     without the filter) are widened to double and projected: the image is sfe_mapset_render2's for xy = the selected
 *     float32 points as doubles.  Refused with SFE_ERR_ARG before anything changes, besides sfe_mapset_render2's refusals: a
 *     store of another context, a handle the store does not hold or whose count is < 0, a frame list for a cloud without
 *     keys (one not built by sfe_cloud_store_get_points_keys[_many] or sfe_cloud_store_put_keys).
 * sfe_remove_outlier_many: sfe_remove_outlier's decision for n_clouds clouds in one launch: cloud c = pts[off[c] .. off[c + 1])
 *   (points), keep_out[i] = 1 for the points that stay.  One synchronisation. */
typedef struct sfe_mapset sfe_mapset;
int sfe_mapset_create(sfe_ctx *ctx, int n_maps, int rows, int cols, int max_keyframes, int max_px, sfe_mapset **out);
void sfe_mapset_destroy(sfe_mapset *ms);
int sfe_mapset_geometry(sfe_mapset *ms, const float *sonar_xy, int img_rows, int img_cols, int *id_out);
int sfe_mapset_set_logodds(sfe_mapset *ms, int n, const int32_t *maps, const int32_t *slots, const int32_t *geoms,
                           const float *logodds);
int sfe_mapset_measure(sfe_mapset *ms, int n, const int32_t *maps, const int32_t *slots, const int32_t *geoms,
                       const int32_t *hit_off, const int32_t *hits, const int32_t *hrhc, const int32_t *k_off,
                       const float *ktab, int n_ktab, const double *div, float miss32, float logit_miss, float hit32,
                       float logit_hit);
int sfe_mapset_measure_stages(sfe_mapset *ms, int b, uint8_t *hits_out, float *prob_out, int32_t *first_hits_out);
int sfe_mapset_hit_table(sfe_mapset *ms, const float *bearings, int num_bearings, const double *breaks, const double *coef,
                         int n_intervals, double margin, int num_ranges, double range_resolution, int range_in_double,
                         int r_skip, int c_skip, int *id_out);
int sfe_mapset_measure_store(sfe_mapset *ms, sfe_cloud_store *store, int n, const int32_t *maps, const int32_t *slots,
                             const int32_t *geoms, const int32_t *handles, const int32_t *tabs, double radius, int min_points,
                             const int32_t *hrhc, const int32_t *k_off, const float *ktab, int n_ktab, const double *div,
                             float miss32, float logit_miss, float hit32, float logit_hit, int32_t *n_points_out,
                             int32_t *n_undecided_out);
int sfe_mapset_measure_store_undecided(sfe_mapset *ms, float *xy_out, int32_t *pos_out, int cap);
int sfe_mapset_measure_store_finish(sfe_mapset *ms, int n_cells, const int32_t *pos, const int32_t *cells);
int sfe_mapset_fit_bounds(sfe_mapset *ms, int n, const int32_t *maps, const int32_t *slots, const double *pose4,
                          const double *origin2, double resolution, int32_t *mm_out);
int sfe_mapset_grow(sfe_mapset *ms, int n, const int32_t *maps, const int32_t *grow4);
int sfe_mapset_refit(sfe_mapset *ms, int n, const int32_t *maps, const int32_t *slots, const double *pose4,
                     const double *origin2, double resolution, const int32_t *mm, const int32_t *shift2, const uint8_t *dec);
int sfe_mapset_cells(sfe_mapset *ms, int map, int slot, uint16_t *r_out, uint16_t *c_out, float *l_out, int cap, int *n_out);
int sfe_mapset_logodds(sfe_mapset *ms, int map, int slot, float *out, int cap);
int sfe_mapset_shape(sfe_mapset *ms, int map, int32_t *rows_cols_grow4);
int sfe_mapset_apply_launches(sfe_mapset *ms, long long *n_out);
int sfe_mapset_read_grid(sfe_mapset *ms, int map, int which, float *out, long long cap);
int sfe_mapset_frames(sfe_mapset *ms, int n_maps, const int32_t *maps, const int32_t *slot_off, const int32_t *slots);
int sfe_mapset_render(sfe_mapset *ms, int n, const int32_t *maps, const int32_t *which, const int32_t *box4,
                      const int32_t *out_hw, const double *inv, const int32_t *resize, const long long *out_off,
                      int8_t *occ_out, long long total);
int sfe_mapset_render2(sfe_mapset *ms, int n, const int32_t *maps, const int32_t *slot_off, const int32_t *slots,
                       const int32_t *box4, const int32_t *pt_off, const double *xy, const int32_t *filter,
                       const double *radius, const int32_t *min_points, const int32_t *dilate_hs, const double *origin2,
                       const double *resolution, const int32_t *out_hw, const double *inv, const int32_t *resize,
                       const long long *out_off, int8_t *occ_out, long long total);
int sfe_mapset_render2_store(sfe_mapset *ms, sfe_cloud_store *store, int n, const int32_t *maps, const int32_t *slot_off,
                             const int32_t *slots, const int32_t *box4, const int32_t *handles, const int32_t *all_frames,
                             const int32_t *frame_off, const int32_t *frames, const int32_t *filter, const double *radius,
                             const int32_t *min_points, const int32_t *dilate_hs, const double *origin2,
                             const double *resolution, const int32_t *out_hw, const double *inv, const int32_t *resize,
                             const long long *out_off, int8_t *occ_out, long long total);
int sfe_remove_outlier_many(sfe_ctx *ctx, const float *pts, const int32_t *off, int n_clouds, double radius, int min_points,
                            uint8_t *keep_out);

/* ---- the intensity mosaic of bruce_slam/mapping.py (pub_intensity: :128-130, :241-243, :272-298, :442-444, :457-459,
 * :498-499).  Off until sfe_mapset_enable_intensity: a set that never enables it allocates, launches and records exactly
 * what it did before these calls existed.  The sfe_map calls are the set's over map 0.
 *   sfe_mapset_enable_intensity: refused with SFE_ERR_ARG once a geometry is registered or a slot is in use.  Per slot the
 *     subsampled ping uint8 [px] and a double-buffered payload uint8 [2][px] next to l (+3 bytes per pixel: the arena
 *     becomes 23 bytes per pixel); per map a uint32 sum grid and a uint16 counter grid of the float grid's shape, zeroed.
 *     From then on sfe_mapset_refit writes i = image[first pixel of the cell] next to l, its applies add / subtract i on
 *     the sum grid and 1 on the counter grid (both wrapping) in the same launches, and sfe_mapset_grow pads both grids with
 *     zeros on all four sides.  A fit of a slot without an image is refused before anything changes.
 *   sfe_mapset_set_intensity: n full-size pings, back to back in `images`, image b for (maps[b], slots[b]) of geometry
 *     geoms[b]; shape4[4 b ..] = {full_rows, full_cols, r_skip, c_skip}.  The slot keeps image[::r_skip, ::c_skip], which
 *     must have the geometry's image shape (SFE_ERR_ARG otherwise; a slot beyond the arena SFE_ERR_CAP; both before anything
 *     changes).  One upload through the pinned staging, one launch; enqueue only.
 *   sfe_mapset_set_intensity_dev: the same from n device pointers, row b of image i at d_images[i] + b * row_stride[i]
 *     (row_stride >= full_cols; full_rows rows must be readable); nothing is uploaded but the job table.
 *   sfe_mapset_render_intensity: get_intensity_grid for n maps in one launch and one read-back: job b writes box4[4 b ..] =
 *     {r0, r1, c0, c1} of map maps[b] at out + out_off[b], `total` bytes in all: -1 where the counter is 0, else
 *     (int8) rint(((double) sum / 255.0) * 100.0 / (double) counter), rint half to even (csrc/sfe_map_intensity.h).
 *   sfe_mapset_read_intensity: the two grids of one map (either pointer may be null), cap cells each.
 *   sfe_mapset_slot_intensity: a slot's subsampled image and the payload i of its current cell list (in the order of
 *     sfe_mapset_cells; any of the three outputs may be null). */
int sfe_mapset_enable_intensity(sfe_mapset *ms);
int sfe_mapset_set_intensity(sfe_mapset *ms, int n, const int32_t *maps, const int32_t *slots, const int32_t *geoms,
                             const int32_t *shape4, const uint8_t *images);
int sfe_mapset_set_intensity_dev(sfe_mapset *ms, int n, const int32_t *maps, const int32_t *slots, const int32_t *geoms,
                                 const int32_t *shape4, const void *const *d_images, const long long *row_stride);
int sfe_mapset_render_intensity(sfe_mapset *ms, int n, const int32_t *maps, const int32_t *box4, const long long *out_off,
                                long long total, int8_t *out);
int sfe_mapset_read_intensity(sfe_mapset *ms, int map, uint32_t *intensity_out, uint16_t *counter_out, long long cap);
int sfe_mapset_slot_intensity(sfe_mapset *ms, int map, int slot, uint8_t *image_out, int image_cap, uint8_t *i_out,
                              int cells_cap, int *n_out);
int sfe_map_enable_intensity(sfe_map *m);
int sfe_map_set_intensity(sfe_map *m, int slot, int geom, int full_rows, int full_cols, int r_skip, int c_skip,
                          const uint8_t *image);
int sfe_map_set_intensity_dev(sfe_map *m, int slot, int geom, int full_rows, int full_cols, int r_skip, int c_skip,
                              const void *d_image, long long row_stride);
int sfe_map_render_intensity(sfe_map *m, int r0, int r1, int c0, int c1, int8_t *out);
int sfe_map_read_intensity(sfe_map *m, uint32_t *intensity_out, uint16_t *counter_out, long long cap);
int sfe_map_slot_intensity(sfe_map *m, int slot, uint8_t *image_out, int image_cap, uint8_t *i_out, int cells_cap, int *n_out);

#ifdef __cplusplus
}
#endif
#endif /* SONARFE_H */
