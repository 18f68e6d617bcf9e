// coarse_ladder.h -- the reference's coarse depths of one ray (render_utils.py:105-129), stated once for the two kernels that
// write them: coarse_z_kernel (render.hip) and the fallback rows of occupancy_coarse_z_kernel (occupancy.hip).  Both files are
// compiled with -ffp-contract=off, so every operation below is rounded on its own in both and the bits cannot differ.
#pragma once
#include <hip/hip_runtime.h>

namespace na {

__device__ __forceinline__ float z_of_t(float near, float far, float t, int lindisp) {
    if (!lindisp) return near * (1.0f - t) + far * t;
    return 1.0f / (1.0f / near * (1.0f - t) + 1.0f / far * t);
}

// Sample s of the Nc-sample ladder of a ray with the given near / far; under perturb the stratified jitter in z-space, with
// `rand` the ray's draw for sample s (not read otherwise).
__device__ __forceinline__ float ladder_z(float near, float far, const float *t_vals, int s, int Nc, int lindisp, int perturb, float rand) {
    float zc = z_of_t(near, far, t_vals[s], lindisp);
    if (perturb) {
        float upper = zc, lower = zc;
        if (s + 1 < Nc) upper = 0.5f * (z_of_t(near, far, t_vals[s + 1], lindisp) + zc);
        if (s > 0) lower = 0.5f * (zc + z_of_t(near, far, t_vals[s - 1], lindisp));
        zc = lower + (upper - lower) * rand;
    }
    return zc;
}

}  // namespace na
