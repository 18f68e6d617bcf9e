// occupancy.hip -- the occupancy grid (include/nerf_amd.h "Occupancy grid"): which points reach the field kernels.  The
// lookup, the sample points a grid is filled from, marking, dilation, the per-view compaction of a pass's sample points and
// its inverse.  Plain memory-bound kernels: integer arithmetic, loads / stores and fp32 operations rounded one by one (this
// file is compiled with -ffp-contract=off), no float atomics and no atomics on the grid -- one thread writes each whole
// word -- so every result is defined exactly and tested for equality, like pixel_select.hip.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "coarse_ladder.h"
#include "kernels.h"
#include "mix32.h"
#include "pipeline.h"

namespace na {

namespace {
constexpr int OC_BLOCK = 256;           // 4 waves of 64; also the points per count of the compaction (launch_compact_scan)

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + OC_BLOCK - 1) / OC_BLOCK); }
inline int launched() { return hipGetLastError() == hipSuccess ? NERF_AMD_OK : NERF_AMD_EHIP; }

// The lookup (nerf_amd.h): the cell of p, or -1 outside.  Two rounded operations per axis; the comparisons are false for NaN.
__device__ __forceinline__ int cell_of(const OccGrid &g, float px, float py, float pz) {
    const float p[3] = {px, py, pz};
    int i[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float d = p[a] - g.lo[a];
        const float t = d * g.scale[a];
        if (!(t >= 0.0f && t < (float)g.n[a])) return -1;
        i[a] = (int)floorf(t);
    }
    return (i[0] * g.n[1] + i[1]) * g.n[2] + i[2];
}

__device__ __forceinline__ bool bit_of(const int32_t *words, int c) { return ((uint32_t)words[c >> 5] >> (c & 31)) & 1u; }

__device__ __forceinline__ bool live_at(const OccGrid &g, int c) { return c < 0 ? g.outside_live != 0 : bit_of(g.words, c); }
}  // namespace

// ---------------------------------------------------------------------------
// The lookup alone: one thread per point.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(OC_BLOCK) void occupancy_query_kernel(OccGrid g, const float *pts, int64_t n, uint8_t *live, int32_t *cell) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int c = cell_of(g, pts[3 * idx], pts[3 * idx + 1], pts[3 * idx + 2]);
    live[idx] = live_at(g, c) ? 1 : 0;
    if (cell) cell[idx] = c;
}

int launch_occupancy_query(const OccGrid &g, const float *pts, int64_t n, uint8_t *live, int32_t *cell, hipStream_t s) {
    if (n <= 0) return NERF_AMD_OK;
    hipLaunchKernelGGL(occupancy_query_kernel, dim3(blocks_for(n)), dim3(OC_BLOCK), 0, s, g, pts, n, live, cell);
    return launched();
}

// ---------------------------------------------------------------------------
// Sample points of cells: one thread per (cell, sample).  Sample 0 the centre, the others the keyed 8-bit lattice jitter.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(OC_BLOCK) void occupancy_sample_kernel(OccGrid g, uint32_t c0, int64_t n, int K, uint32_t seed, float *pts) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const uint32_t j = (uint32_t)(idx % K), c = c0 + (uint32_t)(idx / K);
    const uint32_t nz = (uint32_t)g.n[2], ny = (uint32_t)g.n[1];
    const uint32_t i[3] = {c / (nz * ny), (c / nz) % ny, c % nz};
    uint32_t h[3] = {0, 0, 0};
    if (j > 0) {
        const uint32_t v = mix32(mix32(seed + 0x9e3779b9u * j) ^ c);
        h[0] = v & 255u; h[1] = (v >> 8) & 255u; h[2] = (v >> 16) & 255u;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float f = j > 0 ? ((float)h[a] + 0.5f) * (1.0f / 256.0f) : 0.5f;      // exact: a multiple of 1/512
        const float u = ((float)i[a] + f) * g.width[a];                             // (the sum is exact: 19 bits)
        pts[3 * idx + a] = g.lo[a] + u;
    }
}

int launch_occupancy_sample_points(const OccGrid &g, int64_t c0, int64_t c1, int K, uint32_t seed, float *pts, hipStream_t s) {
    const int64_t n = (c1 - c0) * K;
    if (n <= 0) return NERF_AMD_OK;
    hipLaunchKernelGGL(occupancy_sample_kernel, dim3(blocks_for(n)), dim3(OC_BLOCK), 0, s, g, (uint32_t)c0, n, K, seed, pts);
    return launched();
}

// ---------------------------------------------------------------------------
// Marking: one thread per cell decides its bit, a wave's ballot is two whole words (c0 is a multiple of 32 and a block
// starts a multiple of 64 cells behind it), lanes 0 and 32 store one each.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(OC_BLOCK) void occupancy_mark_kernel(const float *sigma, int64_t c0, int64_t n_cells, int K, float threshold,
                                                                  int accumulate, int32_t *words) {
    const int64_t rel = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;          // cell c0 + rel
    bool on = false;
    if (rel < n_cells) {
        const float *row = sigma + rel * K;
        for (int j = 0; j < K; ++j) on = on || row[j] > threshold;
    }
    const uint64_t ballot = __ballot(on);
    const int lane = threadIdx.x & 63;
    if ((lane & 31) != 0 || rel >= n_cells) return;                             // (a word whose first cell is past c1 is not touched)
    const uint32_t bits = (uint32_t)(ballot >> lane);
    int32_t *w = words + ((c0 + rel) >> 5);
    if (accumulate) *w = (int32_t)((uint32_t)*w | bits);
    else *w = (int32_t)bits;
}

int launch_occupancy_mark(const float *sigma, int64_t c0, int64_t c1, int K, float threshold, int accumulate, int32_t *words,
                          hipStream_t s) {
    const int64_t n = c1 - c0;
    if (n <= 0) return NERF_AMD_OK;
    hipLaunchKernelGGL(occupancy_mark_kernel, dim3(blocks_for(n)), dim3(OC_BLOCK), 0, s, sigma, c0, n, K, threshold, accumulate, words);
    return launched();
}

// ---------------------------------------------------------------------------
// Dilation: `iterations` rounds of a 3 x 3 x 3 maximum with off-grid cells ignored compose, on a box, into ONE maximum over
// the window of reach `iterations` (as in pixel_select.hip's dilate_mask_kernel), so one pass computes it.  One thread per
// output word; the scan of a cell's window stops at the first set bit.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(OC_BLOCK) void occupancy_dilate_kernel(const int32_t *in, int nx, int ny, int nz, int reach, int n_words,
                                                                    int32_t *out) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    const int n_cells = nx * ny * nz;
    uint32_t bits = 0;
    for (int b = 0; b < 32; ++b) {
        const int c = 32 * w + b;
        if (c >= n_cells) break;
        const int z = c % nz, y = (c / nz) % ny, x = c / (nz * ny);
        const int x0 = max(x - reach, 0), x1 = min(x + reach, nx - 1), y0 = max(y - reach, 0), y1 = min(y + reach, ny - 1);
        const int z0 = max(z - reach, 0), z1 = min(z + reach, nz - 1);
        bool on = false;
        for (int xx = x0; xx <= x1 && !on; ++xx)
            for (int yy = y0; yy <= y1 && !on; ++yy) {
                const int base = (xx * ny + yy) * nz;
                for (int zz = z0; zz <= z1 && !on; ++zz) on = bit_of(in, base + zz);
            }
        if (on) bits |= 1u << b;
    }
    out[w] = (int32_t)bits;
}

int launch_occupancy_dilate(const int32_t *in, int nx, int ny, int nz, int reach, int32_t *out, hipStream_t s) {
    const int n_words = (int)(((int64_t)nx * ny * nz + 31) / 32);
    hipLaunchKernelGGL(occupancy_dilate_kernel, dim3(blocks_for(n_words)), dim3(OC_BLOCK), 0, s, in, nx, ny, nz, reach, n_words, out);
    return launched();
}

// ---------------------------------------------------------------------------
// The per-view compaction, after launch_compact_mask: counts per block of 256 points, one scan of the counts, then every
// live point written at its rank.  Stable (point order) by construction: no atomics.  The count pass leaves each point's
// verdict in rank[] (0 live, -1 culled), so the grid is read once per point.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void sample_point(const float *rays, int ray_ch, const float *z, int64_t idx, int S, float p[3], int64_t *ray) {
    *ray = idx / S;
    const float *r = rays + *ray * ray_ch;
    const float zz = z[idx];
    p[0] = mul_then_add(r[3], zz, r[0]);          // pts = o + d z, the product rounded first: the field kernels' own two operations
    p[1] = mul_then_add(r[4], zz, r[1]);
    p[2] = mul_then_add(r[5], zz, r[2]);
}

__global__ __launch_bounds__(OC_BLOCK) void occupancy_cull_count_kernel(OccGrid g, const float *rays, int ray_ch, const float *z, int64_t n,
                                                                        int S, int32_t *rank, int32_t *block_counts) {
    __shared__ int wave_counts[OC_BLOCK / 64];
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool on = false;
    if (idx < n) {
        float p[3];
        int64_t ray;
        sample_point(rays, ray_ch, z, idx, S, p, &ray);
        on = live_at(g, cell_of(g, p[0], p[1], p[2]));
        rank[idx] = on ? 0 : -1;
    }
    const uint64_t ballot = __ballot(on);
    if ((threadIdx.x & 63) == 0) wave_counts[threadIdx.x >> 6] = __popcll(ballot);
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
        for (int w = 0; w < OC_BLOCK / 64; ++w) c += wave_counts[w];
        block_counts[blockIdx.x] = c;
    }
}

__global__ __launch_bounds__(OC_BLOCK) void occupancy_cull_write_kernel(const float *rays, int ray_ch, const float *z, int64_t n, int S,
                                                                        const int32_t *block_offsets, int32_t *rank, float *pts_live,
                                                                        float *vd_live) {
    __shared__ int wave_counts[OC_BLOCK / 64];
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool on = idx < n && rank[idx] == 0;
    const uint64_t ballot = __ballot(on);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_counts[wave] = __popcll(ballot);
    __syncthreads();
    if (!on) return;
    int r = block_offsets[blockIdx.x] + __popcll(ballot & (((uint64_t)1 << lane) - 1));
    for (int w = 0; w < wave; ++w) r += wave_counts[w];
    rank[idx] = r;
    float p[3];
    int64_t ray;
    sample_point(rays, ray_ch, z, idx, S, p, &ray);
    float *dst = pts_live + 3 * (int64_t)r;
    dst[0] = p[0]; dst[1] = p[1]; dst[2] = p[2];
    if (vd_live) {
        const float *v = rays + ray * ray_ch + 8;
        float *dv = vd_live + 3 * (int64_t)r;
        dv[0] = v[0]; dv[1] = v[1]; dv[2] = v[2];
    }
}

int launch_occupancy_cull(const OccGrid &g, const float *rays, int ray_ch, const float *z, int64_t R, int S, int32_t *block_counts,
                          int32_t *rank, float *pts_live, float *vd_live, int64_t *count, hipStream_t s) {
    const int64_t n = R * S;
    const unsigned nb = blocks_for(n);
    if (nb > 0)
        hipLaunchKernelGGL(occupancy_cull_count_kernel, dim3(nb), dim3(OC_BLOCK), 0, s, g, rays, ray_ch, z, n, S, rank, block_counts);
    if (int rc = launch_compact_scan(block_counts, (int)nb, count, s)) return rc;        // (no blocks: writes the zero count)
    if (nb > 0)
        hipLaunchKernelGGL(occupancy_cull_write_kernel, dim3(nb), dim3(OC_BLOCK), 0, s, rays, ray_ch, z, n, S, block_counts, rank, pts_live,
                           vd_live);
    return launched();
}

// ---------------------------------------------------------------------------
// The compaction with a cap (training and pose estimation: a list of fixed capacity, so no count ever reaches the host).
// The count and scan launches are the uncapped ones; the write launch covers max(n, capacity) threads: a live point whose
// rank is below the cap writes its row and src[rank], every other point gets rank -1, and thread i < capacity writes
// padding row i when i >= kept = min(live, capacity).  A row is written by exactly one thread: below `kept` by the live
// point of that rank, from `kept` on by thread i.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(OC_BLOCK) void occupancy_cull_capped_write_kernel(OccGrid g, const float *rays, int ray_ch, const float *z,
                                                                               int64_t n, int S, int64_t capacity,
                                                                               const int32_t *block_offsets, int32_t *rank, int32_t *src,
                                                                               float *pts_live, float *vd_live, int64_t *counts) {
    __shared__ int wave_counts[OC_BLOCK / 64];
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool on = idx < n && rank[idx] == 0;
    const uint64_t ballot = __ballot(on);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_counts[wave] = __popcll(ballot);
    __syncthreads();
    const int64_t live = counts[0];                                   // (the scan's total; this launch only reads it)
    const int64_t kept = live < capacity ? live : capacity;
    if (idx == 0) counts[1] = kept;
    if (idx < capacity && idx >= kept) {
        src[idx] = -1;
        float *dst = pts_live + 3 * idx;
        dst[0] = g.centre[0]; dst[1] = g.centre[1]; dst[2] = g.centre[2];
        if (vd_live) {
            float *dv = vd_live + 3 * idx;
            dv[0] = 0.0f; dv[1] = 0.0f; dv[2] = 1.0f;
        }
    }
    if (!on) return;
    int r = block_offsets[blockIdx.x] + __popcll(ballot & (((uint64_t)1 << lane) - 1));
    for (int w = 0; w < wave; ++w) r += wave_counts[w];
    if (r >= capacity) {
        rank[idx] = -1;
        return;
    }
    rank[idx] = r;
    src[r] = (int32_t)idx;
    float p[3];
    int64_t ray;
    sample_point(rays, ray_ch, z, idx, S, p, &ray);
    float *dst = pts_live + 3 * (int64_t)r;
    dst[0] = p[0]; dst[1] = p[1]; dst[2] = p[2];
    if (vd_live) {
        const float *v = rays + ray * ray_ch + 8;
        float *dv = vd_live + 3 * (int64_t)r;
        dv[0] = v[0]; dv[1] = v[1]; dv[2] = v[2];
    }
}

int launch_occupancy_cull_capped(const OccGrid &g, const float *rays, int ray_ch, const float *z, int64_t R, int S, int64_t capacity,
                                 int32_t *block_counts, int32_t *rank, int32_t *src, float *pts_live, float *vd_live, int64_t *counts,
                                 hipStream_t s) {
    const int64_t n = R * S;
    const unsigned nb = blocks_for(n);
    if (nb > 0)
        hipLaunchKernelGGL(occupancy_cull_count_kernel, dim3(nb), dim3(OC_BLOCK), 0, s, g, rays, ray_ch, z, n, S, rank, block_counts);
    if (int rc = launch_compact_scan(block_counts, (int)nb, counts, s)) return rc;       // (no blocks: writes the zero count)
    hipLaunchKernelGGL(occupancy_cull_capped_write_kernel, dim3(blocks_for(n > capacity ? n : capacity)), dim3(OC_BLOCK), 0, s, g, rays,
                       ray_ch, z, n, S, capacity, block_counts, rank, src, pts_live, vd_live, counts);
    return launched();
}

// ---------------------------------------------------------------------------
// The inverse of the compaction: one thread per dense row; a culled row is +0.0 in every channel.
// ---------------------------------------------------------------------------
template <bool VEC4>
__global__ __launch_bounds__(OC_BLOCK) void occupancy_expand_kernel(const float *raw_live, const int32_t *rank, int64_t n, int ch, float *raw) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int r = rank[idx];
    if constexpr (VEC4) {
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (r >= 0) v = reinterpret_cast<const float4 *>(raw_live)[r];
        reinterpret_cast<float4 *>(raw)[idx] = v;
    } else {
        const float *src = raw_live + (int64_t)r * ch;
        float *dst = raw + idx * ch;
        for (int k = 0; k < ch; ++k) dst[k] = r >= 0 ? src[k] : 0.0f;
    }
}

int launch_occupancy_expand(const float *raw_live, const int32_t *rank, int64_t n, int ch, float *raw, hipStream_t s) {
    if (n <= 0) return NERF_AMD_OK;
    const bool vec4 = ch == 4 && (reinterpret_cast<uintptr_t>(raw_live) & 15) == 0 && (reinterpret_cast<uintptr_t>(raw) & 15) == 0;
    if (vec4)
        hipLaunchKernelGGL(occupancy_expand_kernel<true>, dim3(blocks_for(n)), dim3(OC_BLOCK), 0, s, raw_live, rank, n, ch, raw);
    else
        hipLaunchKernelGGL(occupancy_expand_kernel<false>, dim3(blocks_for(n)), dim3(OC_BLOCK), 0, s, raw_live, rank, n, ch, raw);
    return launched();
}

// ---------------------------------------------------------------------------
// The backward of the expansion: one thread per compact row; a padding row (src < 0) is +0.0 in every channel.
// ---------------------------------------------------------------------------
template <bool VEC4>
__global__ __launch_bounds__(OC_BLOCK) void occupancy_gather_rows_kernel(const float *dense, const int32_t *src, int64_t capacity, int ch,
                                                                         float *live) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= capacity) return;
    const int r = src[idx];
    if constexpr (VEC4) {
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (r >= 0) v = reinterpret_cast<const float4 *>(dense)[r];
        reinterpret_cast<float4 *>(live)[idx] = v;
    } else {
        const float *from = dense + (int64_t)r * ch;
        float *dst = live + idx * ch;
        for (int k = 0; k < ch; ++k) dst[k] = r >= 0 ? from[k] : 0.0f;
    }
}

int launch_occupancy_gather_rows(const float *dense, const int32_t *src, int64_t capacity, int ch, float *live, hipStream_t s) {
    if (capacity <= 0) return NERF_AMD_OK;
    const bool vec4 = ch == 4 && (reinterpret_cast<uintptr_t>(dense) & 15) == 0 && (reinterpret_cast<uintptr_t>(live) & 15) == 0;
    if (vec4)
        hipLaunchKernelGGL(occupancy_gather_rows_kernel<true>, dim3(blocks_for(capacity)), dim3(OC_BLOCK), 0, s, dense, src, capacity, ch, live);
    else
        hipLaunchKernelGGL(occupancy_gather_rows_kernel<false>, dim3(blocks_for(capacity)), dim3(OC_BLOCK), 0, s, dense, src, capacity, ch, live);
    return launched();
}

// ---------------------------------------------------------------------------
// The backward of "pts = o + d z at the kept samples" onto the ray batch: one 64-lane wave per ray (four rays per block).
// Lane l adds the kept samples s = l, l + 64, ... in ascending order into accumulators that start at +0.0, then the
// butterfly v_l = v_l + v_(l xor m) for m = 32, 16, 8, 4, 2, 1 (fp32 addition commutes, so every lane ends with the same
// bits); lane 0 stores.  No atomics: the order is the header's, and a numpy mirror reproduces it.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(OC_BLOCK) void occupancy_ray_grads_kernel(const int32_t *rank, const float *z, const float *g_pts,
                                                                       const float *g_vd, int64_t R, int S, int ray_ch, float *g_rays) {
    const int lane = threadIdx.x & 63;
    const int64_t ray = (int64_t)blockIdx.x * (OC_BLOCK / 64) + (threadIdx.x >> 6);
    if (ray >= R) return;                                             // (whole waves leave: the shuffles below see all 64 lanes)
    float acc[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int s = lane; s < S; s += 64) {
        const int64_t idx = ray * S + s;
        const int r = rank[idx];
        if (r < 0) continue;
        const float zz = z[idx];
        const float *gp = g_pts + 3 * (int64_t)r;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v = gp[k];
            const float vz = v * zz;                                  // rounded before it is added (-ffp-contract=off)
            acc[k] = acc[k] + v;
            acc[3 + k] = acc[3 + k] + vz;
        }
        if (g_vd) {
            const float *gv = g_vd + 3 * (int64_t)r;
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[6 + k] = acc[6 + k] + gv[k];
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[k] = acc[k] + __shfl_xor(acc[k], m, 64);
    if (lane != 0) return;
    float *out = g_rays + ray * ray_ch;
#pragma unroll
    for (int k = 0; k < 6; ++k) out[k] = acc[k];
    out[6] = 0.0f; out[7] = 0.0f;
    if (ray_ch == 11) { out[8] = acc[6]; out[9] = acc[7]; out[10] = acc[8]; }
}

int launch_occupancy_ray_grads(const int32_t *rank, const float *z, const float *g_pts, const float *g_vd, int64_t R, int S, int ray_ch,
                               float *g_rays, hipStream_t s) {
    if (R <= 0) return NERF_AMD_OK;
    hipLaunchKernelGGL(occupancy_ray_grads_kernel, dim3(blocks_for(R * 64)), dim3(OC_BLOCK), 0, s, rank, z, g_pts, g_vd, R, S, ray_ch, g_rays);
    return launched();
}

// ---------------------------------------------------------------------------
// Ray bounds: each ray's [near, far] clipped to the span over which P probes of it look up live.  One 64-lane wave per ray
// (four rays per block, like occupancy_ray_grads_kernel).  A round is 64 consecutive probes,
// one per lane, and its ballot the round's live mask: rounds are walked forward to the first non-zero mask, then backward
// from the end no further than that round (whose mask is kept).  The masks are wave-uniform, so are the loops, and an
// early exit skips only rounds that cannot hold the first / last live probe.  No LDS, no atomics; lanes 0 .. ray_ch - 1
// copy or replace the row.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t probe_round(const OccGrid &g, const float o[3], const float d[3], float near, float w, int k, float inv_p) {
    const float u = ((float)k + 0.5f) * inv_p;                         // exact: P is a power of two
    const float t = mul_then_add(w, u, near);                         // near + w u, the product rounded first
    const float px = mul_then_add(d[0], t, o[0]), py = mul_then_add(d[1], t, o[1]), pz = mul_then_add(d[2], t, o[2]);
    return __ballot(live_at(g, cell_of(g, px, py, pz)));
}

__global__ __launch_bounds__(OC_BLOCK) void occupancy_ray_bounds_kernel(OccGrid g, const float *rays, int ray_ch, int64_t R, int P, int pad,
                                                                        float *rays_out, float *bounds, int32_t *span) {
    const int lane = threadIdx.x & 63;
    const int rounds = P >> 6;
    const float inv_p = 1.0f / (float)P;                              // exact
    const int64_t ray = (int64_t)blockIdx.x * (OC_BLOCK / 64) + (threadIdx.x >> 6);
    if (ray >= R) return;                                             // (whole waves leave: the ballots below see all 64 lanes)
    {
        const float *r = rays + ray * ray_ch;
        const float o[3] = {r[0], r[1], r[2]}, d[3] = {r[3], r[4], r[5]};
        const float near = r[6], far = r[7];
        const float w = far - near;
        int first = -1, last = -1, first_round = 0;
        uint64_t m = 0;
        for (int q = 0; q < rounds; ++q) {
            m = probe_round(g, o, d, near, w, q * 64 + lane, inv_p);
            if (m) {
                first_round = q;
                first = q * 64 + __builtin_ctzll(m);
                break;
            }
        }
        float near2 = near, far2 = far;
        if (first >= 0) {
            for (int q = rounds - 1; q >= first_round; --q) {
                const uint64_t mq = q == first_round ? m : probe_round(g, o, d, near, w, q * 64 + lane, inv_p);
                if (mq) {
                    last = q * 64 + 63 - __builtin_clzll(mq);
                    break;
                }
            }
            const int k0 = max(first - pad, 0), k1 = min(last + pad, P - 1);
            if (k0 > 0) near2 = mul_then_add(w, (float)k0 * inv_p, near);
            if (k1 < P - 1) far2 = mul_then_add(w, (float)(k1 + 1) * inv_p, near);
        }
        if (rays_out && lane < ray_ch) rays_out[ray * ray_ch + lane] = lane == 6 ? near2 : lane == 7 ? far2 : r[lane];
        if (lane < 2) {
            if (bounds) bounds[2 * ray + lane] = lane == 0 ? near2 : far2;
            if (span) span[2 * ray + lane] = lane == 0 ? first : last;
        }
    }
}

int launch_occupancy_ray_bounds(const OccGrid &g, const float *rays, int ray_ch, int64_t R, int probes, int pad, float *rays_out,
                                float *bounds, int32_t *span, hipStream_t s) {
    if (R <= 0) return NERF_AMD_OK;
    hipLaunchKernelGGL(occupancy_ray_bounds_kernel, dim3(blocks_for(R * 64)), dim3(OC_BLOCK), 0, s, g, rays, ray_ch, R, probes, pad, rays_out,
                       bounds, span);
    return launched();
}

// ---------------------------------------------------------------------------
// Coarse depths in each ray's live stretches (nerf_amd.h, nerf_amd_occupancy_coarse_z): the ray-bounds probes, all P of them,
// then the reference's stratified ladder in t mapped through the list of live probes.  One 64-lane wave per ray (four rays
// per block).  Round q's ballot is word q of the ray's P-bit live string; lane q keeps it, so the string lies one 64-bit
// word per lane (lanes >= P / 64 hold 0) and never leaves the registers: NO LDS (0 bytes per block), no atomics, no global
// scratch.  Padding ORs the string with itself shifted by 1 .. pad either way, by doubling (at most 13 steps a direction),
// a shift taking its carries from the neighbouring lanes' words.  Popcount per word, an inclusive wave prefix sum, and then
// lane l maps samples s = l, l + 64, ...: a binary search of the prefix sums for the word that holds rank j, and of that
// word's popcounts for its bit.  Every loop around a ballot or a shuffle is wave-uniform (the sample loop runs all 64 lanes,
// a lane past N_samples works on the last sample and stores nothing).  A miss and an all-live ray are the shared ladder.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t word_at(uint64_t x, int lane, int delta) {      // word lane + delta of the string, 0 past either end
    const int src = lane + delta;
    const uint64_t v = __shfl(x, src & 63, 64);
    return (src >= 0 && src < 64) ? v : 0;
}

template <bool UP>
__device__ __forceinline__ uint64_t shift_string(uint64_t x, int lane, int s) {     // the string moved s bits (1 <= s <= 4096) up / down
    const int ws = s >> 6, bs = s & 63;
    const uint64_t a = word_at(x, lane, UP ? -ws : ws), b = word_at(x, lane, UP ? -ws - 1 : ws + 1);
    if (bs == 0) return a;
    return UP ? (a << bs) | (b >> (64 - bs)) : (a >> bs) | (b << (64 - bs));
}

__global__ __launch_bounds__(OC_BLOCK) void occupancy_coarse_z_kernel(OccGrid g, const float *rays, int ray_ch, const float *t_vals,
                                                                      const float *t_rand, int64_t R, int Nc, int P, int pad, int perturb,
                                                                      float *z, int32_t *live_count) {
    const int lane = threadIdx.x & 63;
    const int rounds = P >> 6;
    const float inv_p = 1.0f / (float)P;                              // exact
    const int64_t ray = (int64_t)blockIdx.x * (OC_BLOCK / 64) + (threadIdx.x >> 6);
    if (ray >= R) return;                                             // (whole waves leave: the ballots and shuffles below see all 64 lanes)
    const float *r = rays + ray * ray_ch;
    const float o[3] = {r[0], r[1], r[2]}, d[3] = {r[3], r[4], r[5]};
    const float near = r[6], far = r[7];
    const float w = far - near;
    uint64_t bits = 0;
    for (int q = 0; q < rounds; ++q) {
        const uint64_t m = probe_round(g, o, d, near, w, q * 64 + lane, inv_p);
        if (lane == q) bits = m;
    }
    if (pad > 0) {
        uint64_t up = bits, down = bits;                              // the OR over shifts 0 .. covered, each way
        for (int covered = 0; covered < pad;) {
            const int step = min(covered + 1, pad - covered);
            up |= shift_string<true>(up, lane, step);
            down |= shift_string<false>(down, lane, step);
            covered += step;
        }
        bits = lane < rounds ? (up | down) : 0;                       // (what was pushed past probe P - 1 is dropped)
    }
    int incl = __popcll(bits);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const int below = __shfl_up(incl, m, 64);
        if (lane >= m) incl += below;
    }
    const int L = __shfl(incl, 63, 64);
    if (live_count && lane == 0) live_count[ray] = L;
    float *zr = z + ray * Nc;
    const float *rand = perturb ? t_rand + ray * Nc : nullptr;
    if (L == 0 || L == P) {                                           // a miss, or nothing to drop: the reference ladder
        for (int s = lane; s < Nc; s += 64) zr[s] = ladder_z(near, far, t_vals, s, Nc, 0, perturb, perturb ? rand[s] : 0.0f);
        return;
    }
    const float fl = (float)L;
    for (int s0 = 0; s0 < Nc; s0 += 64) {
        const int s = min(s0 + lane, Nc - 1);
        float t = t_vals[s];
        if (perturb) {
            float upper = t, lower = t;
            if (s > 0) lower = 0.5f * (t + t_vals[s - 1]);
            if (s < Nc - 1) upper = 0.5f * (t_vals[s + 1] + t);
            t = lower + (upper - lower) * rand[s];
        }
        const float a = fminf(t * fl, fl);
        const int j = min((int)floorf(a), L - 1);
        const float f = a - (float)j;
        int k = 0;                                                    // the word that holds rank j: the number of words with incl <= j
#pragma unroll
        for (int step = 32; step >= 1; step >>= 1)
            if (__shfl(incl, k + step - 1, 64) <= j) k += step;
        const uint64_t m = __shfl(bits, k, 64);
        int rank = j - (__shfl(incl, k, 64) - __popcll(m));           // ... and the rank of the bit inside it
        int pos = 0;
#pragma unroll
        for (int width = 32; width >= 1; width >>= 1) {
            const int c = __popcll((m >> pos) & (((uint64_t)1 << width) - 1));
            if (rank >= c) { rank -= c; pos += width; }
        }
        const float e = (float)(k * 64 + pos) + f;
        const float u = e * inv_p;                                    // exact
        if (s0 + lane < Nc) zr[s0 + lane] = mul_then_add(w, u, near);
    }
}

int launch_occupancy_coarse_z(const OccGrid &g, const float *rays, int ray_ch, const float *t_vals, const float *t_rand, int64_t R, int Nc,
                              int probes, int pad, int perturb, float *z, int32_t *live_count, hipStream_t s) {
    if (R <= 0) return NERF_AMD_OK;
    hipLaunchKernelGGL(occupancy_coarse_z_kernel, dim3(blocks_for(R * 64)), dim3(OC_BLOCK), 0, s, g, rays, ray_ch, t_vals, t_rand, R, Nc,
                       probes, pad, perturb, z, live_count);
    return launched();
}

}  // namespace na
