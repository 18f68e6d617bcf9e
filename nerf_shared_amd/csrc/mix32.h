// mix32.h -- the 32-bit mixing function of the keyed draws (include/nerf_amd.h: mix() of nerf_amd_draw_pixels and of
// nerf_amd_occupancy_sample_points).  uint32 arithmetic mod 2^32.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace na {

__host__ __device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

}  // namespace na
