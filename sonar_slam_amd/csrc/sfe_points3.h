// Device helpers for clouds of packed float triples (12-byte stride, a contiguous N x 3 float32 array), shared by the N x 3
// cloud functions (sfe_pcl3.hip), the octree downsample (sfe_octree3.hip), the 3-D keyframe store (sfe_store3.hip) and the
// 3-D ICP (sfe_icp3.hip): the squared distance, the LDS tile and the nearest-point scan over it.
#pragma once
#include "sfe_icp_common.h"

#define P3_TILE 2048 // points per LDS tile (24 KiB)

// d2 = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)), no fma; a z of 0 on both sides adds +0 and leaves the 2-D value
__device__ __forceinline__ float p3_dist2(float px, float py, float pz, float tx, float ty, float tz)
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

// The nearest of pts[0 .. n) to (px, py, pz) by p3_dist2 -> (best, bi), (+inf, -1) if there is none: the cloud goes through
// the tile s[3 P3_TILE] and every lane reads the same LDS words (a broadcast).  The update is on strict `<` in ascending index
// with the best carried from tile to tile: ties go to the lowest index, across tile borders too; NaN and +inf never win.
// Called by all 256 threads of the workgroup (it holds the tile's barriers).
__device__ __forceinline__ void p3_nearest(float *s, const float *__restrict__ pts, int n, float px, float py, float pz,
                                           float &best_out, int &bi_out)
{
    float best = INFINITY; // (locals, not the references: the scan keeps them in registers whatever `s` may alias)
    int bi = -1;
    for (int tb = 0; tb < n; tb += P3_TILE) {
        const int tn = min(P3_TILE, n - tb);
        __syncthreads();
        p3_stage(s, pts, tb, tn);
        __syncthreads();
        for (int j = 0; j < tn; ++j) {
            const float d = p3_dist2(px, py, pz, s[3 * j], s[3 * j + 1], s[3 * j + 2]);
            if (d < best) {
                best = d;
                bi = tb + j;
            }
        }
    }
    best_out = best;
    bi_out = bi;
}
