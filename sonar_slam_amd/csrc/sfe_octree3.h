// The 3-D octree downsample (sfe_octree3.hip: pcl.downsample on N x 3, many clouds per launch) as enqueue-only steps.  Its
// callers: pcl.downsample on N x 3 (sfe_downsample3 in sfe_pcl3.hip, a one-job call), CloudStore3.get_points (sfe_store3.hip)
// and the octree stage of a 3-D ICP chain (sfe_icp3_dpf.hip).  This header names what a caller hands the kernels.
#pragma once
#include "sfe_internal.h"
#include "sfe_store3_slots.h"

#define S3_MAX_LEVELS 21  // 3 key bits per level in a 64-bit key; a deeper tree is cut here
#define S3_MAX_JOBS 65535 // blockIdx.y

struct S3Header { // a job's tree and its leaf count
    float cx, cy, cz, radius;
    int levels;
    int n_seg;
};

// device scratch of one downsample over concatenations of `total` points in all (n_jobs jobs)
struct S3OctreeBufs {
    unsigned long long *keys, *skeys; // [total] each
    int *sidx;                        // [total]
    int *seg;                         // [total + n_jobs]
    S3Header *hdr;                    // [n_jobs]
    float *out;                       // [total][3]: job j's medoids from its `cat` on, in leaf order
    int *midx;                        // [total] or nullptr: the medoids' indices in their concatenations
};

// std::to_string(float) and back (pcl.cpp:134): the leaf size the reference's octree is built with
float sfe_s3_max_size(float resolution);

// bounding box -> keys -> ranks -> segments -> medoids of the jobs d_jobs[0 .. n_jobs) (n_jobs <= S3_MAX_JOBS) over d_cat; job
// j reads its tot points at d_jobs[j].cat, tot read ON THE DEVICE (max_tot: an upper bound known to the host, sizes the
// grids), and leaves hdr[j].n_seg medoids.  One launch per step.
int sfe_s3_octree_enqueue(sfe_ctx *ctx, const float *d_cat, const S3Job *d_jobs, int n_jobs, int max_tot, float max_size,
                          const S3OctreeBufs &b);

// every job's size (raw: its tot, else its hdr n_seg) to d_cnt, the exclusive sum of the sizes in front of it to d_off
// (all n_jobs jobs, one workgroup) ...
int sfe_s3_offsets_enqueue(sfe_ctx *ctx, const S3Job *d_jobs, const S3Header *d_hdr, int n_jobs, int raw, int *d_cnt,
                           long long *d_off);
// ... and the jobs' points from their `cat` in d_from to pool[top + d_off[j] ..), one behind the other (n_jobs <= S3_MAX_JOBS)
int sfe_s3_place_enqueue(sfe_ctx *ctx, const float *d_from, const S3Job *d_jobs, int n_jobs, int max_tot, const int *d_cnt,
                         const long long *d_off, long long top, float *pool);
