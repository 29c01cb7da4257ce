// The MinDist / MedianDist outlier filters' rules (sfe_icp_outliers), one copy for the 2-D kernels (sfe_icp_common.h), the
// 3-D ones (sfe_icp3_chain.h) and the CPU check of the latter (tests/host/icp3_chain_check.cpp): host and device.
#pragma once
#include "../../include/sonarfe.h"

#if defined(__HIPCC__)
#define SFE_ICP_OX_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SFE_ICP_OX_HD inline
#endif

// MedianDistOutlierFilter: rank (0-based) of the median among the nfin finite distances -- Matches::getDistsQuantile(0.5)
// as the trimmed quantile is taken: values.size() * 0.5 in float, truncated.  (One float product, which nothing can be
// fused into: the plain operator rounds as __fmul_rn does.)
SFE_ICP_OX_HD unsigned icp_median_rank(unsigned nfin) { return (unsigned)((float)nfin * 0.5f); }

// kept by MinDist (d >= minDist^2, min2 = fl(minDist minDist)) and by the median filter (d <= med_limit = fl(factor median))?
SFE_ICP_OX_HD bool icp_ox_keep(const sfe_icp_outliers &O, float min2, float med_limit, float d)
{
    return (!O.use_min_dist || d >= min2) && (!O.use_median || d <= med_limit);
}
