// One cell of the published intensity mosaic (bruce_slam mapping.py:283-285), shared by mapset_render_intensity_kernel
// (sfe_map.hip) and the host check tests/host/map_intensity_check.cpp, which holds it to numpy's expression on the CPU.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SFE_MAP_INTENSITY_HD __host__ __device__ __forceinline__
#else
#define SFE_MAP_INTENSITY_HD inline
#endif

// -1 where nothing was counted, else np.int8(np.round(I / 255.0 * 100.0 / cnt)): float64, in that order, every operation
// correctly rounded (there is no multiply feeding an add, so nothing can be contracted), rint = half to even.  The value
// is at most 100 while I <= 255 * cnt, which holds until a uint32 sum wraps.
SFE_MAP_INTENSITY_HD int8_t sfe_map_intensity_value(uint32_t intensity, uint16_t counter)
{
    if (counter == 0)
        return (int8_t)-1;
    const double q = ((double)intensity / 255.0) * 100.0 / (double)counter;
    return (int8_t)(int)rint(q);
}
