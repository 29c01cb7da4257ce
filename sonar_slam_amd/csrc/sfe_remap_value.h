// The remap decode shared by the remap kernels (sfe_remap.hip) and the dense pass of the extraction (sfe_extract.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "sfe_geom_tables.h" // SFE_CODE_NONE

// Decode one Cartesian pixel.  `rcp` = ceil(2^32 / (pcols+1)) turns the divide of the packed
// linear index into one v_mul_hi (exact for lin < 2^22, checked at geometry creation).
__device__ __forceinline__ int remap_value(const uint8_t *__restrict__ src, int prows, int pcols, unsigned rcp,
                                           uint32_t code)
{
    const unsigned lin = code >> 10;
    const int fy = (int)((code >> 5) & 31u), fx = (int)(code & 31u);
    const unsigned q = __umulhi(lin, rcp);
    const int iy = (int)q - 1, ix = (int)(lin - q * (unsigned)(pcols + 1)) - 1;
    // branch-free taps: clamp the coordinates (always a valid address, all four loads in flight
    // together) and zero the out-of-image ones afterwards (BORDER_CONSTANT 0)
    const int ya = max(iy, 0), yb = min(iy + 1, prows - 1), xa = max(ix, 0), xb = min(ix + 1, pcols - 1);
    const uint8_t *ra = src + (size_t)ya * pcols, *rb = src + (size_t)yb * pcols;
    const int my0 = (iy >= 0) ? 0xff : 0, my1 = (iy + 1 < prows) ? 0xff : 0;
    const int mx0 = (ix >= 0) ? 0xff : 0, mx1 = (ix + 1 < pcols) ? 0xff : 0;
    const int v00 = ra[xa] & my0 & mx0;
    const int v01 = ra[xb] & my0 & mx1;
    const int v10 = rb[xa] & my1 & mx0;
    const int v11 = rb[xb] & my1 & mx1;
    if ((v00 | v01 | v10 | v11) == 0)
        return 0; // sparse detection masks: most taps are empty
    int w00 = (32 - fy) * (32 - fx) * 32, w01 = (32 - fy) * fx * 32;
    int w10 = fy * (32 - fx) * 32, w11 = fy * fx * 32;
    if ((fx | fy) == 0) {
        w00 = 32767;
        w11 = 1;
    }
    const int acc = w00 * v00 + w01 * v01 + w10 * v10 + w11 * v11;
    return (acc + 16384) >> 15; // <= 255 because the weights sum to 32768
}
