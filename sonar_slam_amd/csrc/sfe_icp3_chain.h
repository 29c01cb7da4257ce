// The pieces of a 3-D ICP chain that need no device (sfe_icp3_dpf.hip, sfe_icp3.hip): the data-point stage predicates, the
// outlier filters' keep test, the Bound checker's test and the validation of a stage list.  Host and device, so that
// tests/host/icp3_chain_check.cpp can run them on the CPU; include/sonarfe.h at sfe_icp3_filter_clouds_dev and
// sfe_icp3_compute_jobs_chain_ext states the rules.
//
// Every float product and sum is rounded on its own: __fmul_rn / __fadd_rn on the device, plain operators on the host, which
// is compiled without contraction (-ffp-contract=off).  sqrtf is the correctly rounded one on both.
#pragma once
#include <math.h>

#include "../../include/sonarfe.h"
#include "sfe_icp3_solve.h"
#include "sfe_icp_outlier_rules.h" // the outlier filters' keep test: icp_median_rank, icp_ox_keep (the 2-D chain's)

SFE_ICP3_HD float icp3c_mul(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn(a, b);
#else
    return a * b;
#endif
}

SFE_ICP3_HD float icp3c_add(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(a, b);
#else
    return a + b;
#endif
}

// sqrtf(fl(fl(fl(x x) + fl(y y)) + fl(z z))): with z = 0 the 2-D stage's norm
SFE_ICP3_HD float icp3_dpf_norm(float x, float y, float z)
{
    return sqrtf(icp3c_add(icp3c_add(icp3c_mul(x, x), icp3c_mul(y, y)), icp3c_mul(z, z)));
}

// does the predicate stage s (MAX_DIST, MIN_DIST, BOUNDING_BOX) keep the point?  Strict comparisons: a NaN coordinate fails
// them (a box with remove_inside keeps it, as "not inside").
SFE_ICP3_HD bool icp3_dpf_keep(const sfe_icp_dpf &s, float x, float y, float z)
{
    if (s.kind == SFE_DPF_BOUNDING_BOX) {
        const bool inside = s.f[0] < x && x < s.f[1] && s.f[2] < y && y < s.f[3] && s.f[4] < z && z < s.f[5];
        return inside != (s.remove_inside != 0);
    }
    const bool max = s.kind == SFE_DPF_MAX_DIST;
    if (s.dim < 0) {
        const float norm = icp3_dpf_norm(x, y, z);
        return max ? norm < fabsf(s.f[0]) : norm > fabsf(s.f[0]);
    }
    const float v = s.dim == 0 ? x : s.dim == 1 ? y : z;
    return max ? v < s.f[0] : fabsf(v) > fabsf(s.f[0]);
}

// A stage list of a 3-D chain: ICP3_DPF_OK, or the reason with *bad = the stage (n itself for a bad count or pointer)
enum { ICP3_DPF_OK = 0, ICP3_DPF_COUNT = 1, ICP3_DPF_DIM = 2, ICP3_DPF_OCTREE_SIZE = 3, ICP3_DPF_KIND = 4 };

inline int icp3_dpf_validate(const sfe_icp_dpf *st, int n, int *bad)
{
    *bad = n;
    if (n < 0 || n > SFE_DPF_MAX_STAGES || (n > 0 && !st))
        return ICP3_DPF_COUNT;
    for (int i = 0; i < n; ++i) {
        const sfe_icp_dpf &s = st[i];
        *bad = i;
        if (s.kind == SFE_DPF_MAX_DIST || s.kind == SFE_DPF_MIN_DIST) {
            if (s.dim < -1 || s.dim > 2)
                return ICP3_DPF_DIM;
        } else if (s.kind == SFE_DPF_OCTREE_GRID) {
            if (!(s.f[0] > 0.0f) || !(s.f[0] <= 3.402823466e+38f)) // (NaN, <= 0, inf)
                return ICP3_DPF_OCTREE_SIZE;
        } else if (s.kind != SFE_DPF_BOUNDING_BOX) {
            return ICP3_DPF_KIND;
        }
    }
    *bad = n;
    return ICP3_DPF_OK;
}

// The outlier filters' median rank and keep test under this header's names: the one pair of sfe_icp_outlier_rules.h
SFE_ICP3_HD unsigned icp3_median_rank(unsigned nfin) { return icp_median_rank(nfin); }
SFE_ICP3_HD bool icp3_ox_keep(const sfe_icp_outliers &O, float min2, float med_limit, float d)
{
    return icp_ox_keep(O, min2, med_limit, d);
}

// BoundTransformationChecker on T_iter (4 x 4 row-major floats), in fp64 from the float entries: the rotation is the angle
// between the rotation block and the identity as the Differential checker measures it (icp3_rot_dist), the translation
// sqrt((tx tx + ty ty) + tz tz).  A NaN is never out of bounds.
SFE_ICP3_HD double icp3_bound_rot(const float *T16)
{
    const float R[9] = {T16[0], T16[1], T16[2], T16[4], T16[5], T16[6], T16[8], T16[9], T16[10]};
    const float I[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    return icp3_rot_dist(R, I);
}

SFE_ICP3_HD double icp3_bound_trans(const float *T16)
{
    const double tx = T16[3], ty = T16[7], tz = T16[11];
    return sqrt((tx * tx + ty * ty) + tz * tz);
}

SFE_ICP3_HD bool icp3_bound_out(const sfe_icp_outliers &O, const float *T16)
{
    return icp3_bound_rot(T16) > (double)O.max_rotation_norm || icp3_bound_trans(T16) > (double)O.max_translation_norm;
}
