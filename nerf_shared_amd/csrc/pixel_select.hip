// pixel_select.hip -- which pixels a pose-estimation step looks at (demo_est_rel_pose.py:35-47 and :75-79), on the device:
// interest points of the sensor image, the dilated interest region, its pixel list, and the per-step draw of n distinct
// pixels with their colours.  Integer arithmetic and plain loads / stores throughout: every result is defined exactly
// (include/nerf_amd.h) and tested for equality.  Small latency-bound kernels; one thread per pixel or per drawn slot.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "mix32.h"

namespace na {

namespace {
constexpr int PS_BLOCK = 256;           // 4 waves of 64

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + PS_BLOCK - 1) / PS_BLOCK); }
inline int launched() { return hipGetLastError() == hipSuccess ? NERF_AMD_OK : NERF_AMD_EHIP; }
}  // namespace

// ---------------------------------------------------------------------------
// The draw: a keyed bijection of [0, M) evaluated at slots 0..n-1.
// ---------------------------------------------------------------------------
// One thread per slot: a four-round Feistel network on 2b bits, walked along its cycle until it lands below M (the walk
// starts below M, so it returns there), then the pixel of that index and its colour.  The counter is only read here; the
// one-thread kernel behind this one in the stream advances it, so no block sees a half-advanced value.
__global__ __launch_bounds__(PS_BLOCK) void draw_pixels_kernel(uint32_t M, int n, uint32_t seed, int b, const int64_t *draw_count,
                                                               const int32_t *region, int W, const float *image, int64_t row_stride,
                                                               int C, int32_t *pixels, float *target) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t draw = (uint32_t)(uint64_t)draw_count[0];
    uint32_t key[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) key[r] = mix32(mix32(seed + 0x9e3779b9u * (uint32_t)(r + 1)) ^ draw);
    const uint32_t mask = (1u << b) - 1u;
    uint32_t x = (uint32_t)i;
    do {
        uint32_t L = x >> b, R = x & mask;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t t = L ^ (mix32(R ^ key[r]) & mask);
            L = R;
            R = t;
        }
        x = (L << b) | R;
    } while (x >= M);
    int px, py;
    if (region) {
        px = region[2 * (int64_t)x];
        py = region[2 * (int64_t)x + 1];
    } else {
        px = (int)(x % (uint32_t)W);
        py = (int)(x / (uint32_t)W);
    }
    pixels[2 * i] = px;
    pixels[2 * i + 1] = py;
    const float *src = image + (int64_t)py * row_stride + (int64_t)px * C;
    target[3 * i] = src[0];
    target[3 * i + 1] = src[1];
    target[3 * i + 2] = src[2];
}

__global__ __launch_bounds__(64) void advance_draw_count_kernel(int64_t *draw_count) {
    if (blockIdx.x == 0 && threadIdx.x == 0) draw_count[0] += 1;
}

int launch_draw_pixels(int64_t M, int n, uint32_t seed, int64_t *draw_count, const int32_t *region, int W, const float *image,
                       int64_t row_stride, int C, int32_t *pixels, float *target, hipStream_t s) {
    int bits = 0;                                           // bit_length(M - 1)
    for (uint64_t v = (uint64_t)(M - 1); v; v >>= 1) ++bits;
    int b = (bits + 1) / 2;
    if (b < 1) b = 1;
    if (n > 0) {
        hipLaunchKernelGGL(draw_pixels_kernel, dim3(blocks_for(n)), dim3(PS_BLOCK), 0, s, (uint32_t)M, n, seed, b, draw_count, region, W,
                           image, row_stride, C, pixels, target);
        if (launched() != NERF_AMD_OK) return NERF_AMD_EHIP;
    }
    hipLaunchKernelGGL(advance_draw_count_kernel, dim3(1), dim3(64), 0, s, draw_count);
    return launched();
}

// ---------------------------------------------------------------------------
// Interest points: exact integer Harris (the built-in stand-in for the demo's SIFT detector).
// ---------------------------------------------------------------------------
__device__ __forceinline__ int gray_at(const uint8_t *img, int W, int C, int y, int x) {
    const uint8_t *p = img + ((int64_t)y * W + x) * C;
    return (4899 * (int)p[0] + 9617 * (int)p[1] + 1868 * (int)p[2] + 8192) >> 14;
}

// 3x3 Sobel of the gray image at clamped coordinates -> (gx, gy) per pixel; thread 0 also zeroes the maximum.
__global__ __launch_bounds__(PS_BLOCK) void harris_gradient_kernel(const uint8_t *img, int H, int W, int C, int32_t *gx, int32_t *gy,
                                                                   unsigned long long *max_resp) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx == 0) max_resp[0] = 0ull;
    if (idx >= (int64_t)H * W) return;
    const int y = (int)(idx / W), x = (int)(idx % W);
    const int ym = clampi(y - 1, H - 1), yp = clampi(y + 1, H - 1), xm = clampi(x - 1, W - 1), xp = clampi(x + 1, W - 1);
    const int a = gray_at(img, W, C, ym, xm), b = gray_at(img, W, C, ym, x), c = gray_at(img, W, C, ym, xp);
    const int d = gray_at(img, W, C, y, xm), f = gray_at(img, W, C, y, xp);
    const int g = gray_at(img, W, C, yp, xm), h = gray_at(img, W, C, yp, x), k = gray_at(img, W, C, yp, xp);
    gx[idx] = (c + 2 * f + k) - (a + 2 * d + g);
    gy[idx] = (g + 2 * h + k) - (a + 2 * b + c);
}

// Sums of gx^2, gy^2, gx gy over the 5x5 window at clamped coordinates, the response in int64, and its maximum (an
// integer atomic max is independent of the order of arrival; one atomic per wave).
__global__ __launch_bounds__(PS_BLOCK) void harris_response_kernel(const int32_t *gx, const int32_t *gy, int H, int W, int64_t *resp,
                                                                   unsigned long long *max_resp) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    long long r = 0;
    if (idx < (int64_t)H * W) {
        const int y = (int)(idx / W), x = (int)(idx % W);
        long long sxx = 0, syy = 0, sxy = 0;
        for (int dy = -2; dy <= 2; ++dy) {
            const int64_t row = (int64_t)clampi(y + dy, H - 1) * W;
            for (int dx = -2; dx <= 2; ++dx) {
                const int64_t q = row + clampi(x + dx, W - 1);
                const long long u = gx[q], v = gy[q];
                sxx += u * u;
                syy += v * v;
                sxy += u * v;
            }
        }
        r = 25 * (sxx * syy - sxy * sxy) - (sxx + syy) * (sxx + syy);
        resp[idx] = r;
    }
    unsigned long long m = r > 0 ? (unsigned long long)r : 0ull;        // only positive responses can be interest points
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(m, off, 64);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(max_resp, m);
}

__global__ __launch_bounds__(PS_BLOCK) void harris_select_kernel(const int64_t *resp, int H, int W, int quality,
                                                                 const unsigned long long *max_resp, uint8_t *mask) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)H * W) return;
    const int y = (int)(idx / W), x = (int)(idx % W);
    const long long r = resp[idx];
    bool on = r > 0 && 100 * r >= (long long)quality * (long long)max_resp[0];
    for (int dy = -1; dy <= 1 && on; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= H) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = x + dx;
            if (xx < 0 || xx >= W || (dy == 0 && dx == 0)) continue;
            const long long o = resp[(int64_t)yy * W + xx];
            const bool earlier = dy < 0 || (dy == 0 && dx < 0);       // row-major order: ties go to the first of the equals
            if (earlier ? !(r > o) : !(r >= o)) on = false;
        }
    }
    mask[idx] = on ? 1 : 0;
}

int launch_interest_points(const uint8_t *image, int H, int W, int C, int quality, void *workspace, uint8_t *mask, hipStream_t s) {
    const int64_t n = (int64_t)H * W;
    unsigned long long *max_resp = static_cast<unsigned long long *>(workspace);
    int64_t *resp = reinterpret_cast<int64_t *>(max_resp + 1);
    int32_t *gx = reinterpret_cast<int32_t *>(resp + n), *gy = gx + n;
    hipLaunchKernelGGL(harris_gradient_kernel, dim3(blocks_for(n)), dim3(PS_BLOCK), 0, s, image, H, W, C, gx, gy, max_resp);
    hipLaunchKernelGGL(harris_response_kernel, dim3(blocks_for(n)), dim3(PS_BLOCK), 0, s, gx, gy, H, W, resp, max_resp);
    hipLaunchKernelGGL(harris_select_kernel, dim3(blocks_for(n)), dim3(PS_BLOCK), 0, s, resp, H, W, quality, max_resp, mask);
    return launched();
}

// ---------------------------------------------------------------------------
// Dilation: `iterations` passes of a k x k maximum, anchor at k / 2, off-image pixels ignored.  Because the image is a box
// and the window contains its anchor, the passes compose into ONE maximum over the window [-I a, I (k - 1 - a)] (every
// in-image offset of the composed window is reached through in-image intermediate pixels), so one pass computes it.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(PS_BLOCK) void dilate_mask_kernel(const uint8_t *in, int H, int W, int lo, int hi, uint8_t *out) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)H * W) return;
    const int y = (int)(idx / W), x = (int)(idx % W);
    const int y0 = max(y - lo, 0), y1 = min(y + hi, H - 1), x0 = max(x - lo, 0), x1 = min(x + hi, W - 1);
    int m = 0;
    for (int yy = y0; yy <= y1; ++yy)
        for (int xx = x0; xx <= x1; ++xx) m = max(m, (int)in[(int64_t)yy * W + xx]);
    out[idx] = (uint8_t)m;
}

int launch_dilate_mask(const uint8_t *in, int H, int W, int k, int iterations, uint8_t *out, hipStream_t s) {
    const int a = k / 2;
    hipLaunchKernelGGL(dilate_mask_kernel, dim3(blocks_for((int64_t)H * W)), dim3(PS_BLOCK), 0, s, in, H, W, iterations * a,
                       iterations * (k - 1 - a), out);
    return launched();
}

// ---------------------------------------------------------------------------
// Compaction: counts per block of 256 pixels, an exclusive scan of the counts, then every set pixel written at its rank.
// Stable (row-major order) by construction: no atomics.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(PS_BLOCK) void compact_count_kernel(const uint8_t *mask, int64_t n, int32_t *block_counts) {
    __shared__ int wave_counts[PS_BLOCK / 64];
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool on = idx < n && mask[idx] != 0;
    const uint64_t ballot = __ballot(on);
    if ((threadIdx.x & 63) == 0) wave_counts[threadIdx.x >> 6] = __popcll(ballot);
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
        for (int w = 0; w < PS_BLOCK / 64; ++w) c += wave_counts[w];
        block_counts[blockIdx.x] = c;
    }
}

// One block: thread t owns a contiguous run of the counts; run sums are scanned in LDS, then each run is rewritten as
// exclusive offsets.  Writes the total.
__global__ __launch_bounds__(PS_BLOCK) void compact_scan_kernel(int32_t *block_counts, int n_blocks, int64_t *count) {
    __shared__ int run_sum[PS_BLOCK];
    const int per = (n_blocks + PS_BLOCK - 1) / PS_BLOCK;
    const int first = min((int)threadIdx.x * per, n_blocks), last = min(first + per, n_blocks);
    int sum = 0;
    for (int i = first; i < last; ++i) sum += block_counts[i];
    run_sum[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int t = 0; t < PS_BLOCK; ++t) {
            const int v = run_sum[t];
            run_sum[t] = acc;
            acc += v;
        }
        count[0] = acc;
    }
    __syncthreads();
    int acc = run_sum[threadIdx.x];
    for (int i = first; i < last; ++i) {
        const int v = block_counts[i];
        block_counts[i] = acc;
        acc += v;
    }
}

__global__ __launch_bounds__(PS_BLOCK) void compact_write_kernel(const uint8_t *mask, int64_t n, int W, const int32_t *block_offsets,
                                                                 int32_t *list) {
    __shared__ int wave_counts[PS_BLOCK / 64];
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool on = idx < n && mask[idx] != 0;
    const uint64_t ballot = __ballot(on);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_counts[wave] = __popcll(ballot);
    __syncthreads();
    if (!on) return;
    int rank = block_offsets[blockIdx.x] + __popcll(ballot & (((uint64_t)1 << lane) - 1));
    for (int w = 0; w < wave; ++w) rank += wave_counts[w];
    list[2 * (int64_t)rank] = (int)(idx % W);
    list[2 * (int64_t)rank + 1] = (int)(idx / W);
}

int launch_compact_scan(int32_t *block_counts, int n_blocks, int64_t *count, hipStream_t s) {
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(PS_BLOCK), 0, s, block_counts, n_blocks, count);
    return launched();
}

int launch_compact_mask(const uint8_t *mask, int H, int W, int32_t *block_counts, int32_t *list, int64_t *count, hipStream_t s) {
    const int64_t n = (int64_t)H * W;
    const unsigned nb = blocks_for(n);
    hipLaunchKernelGGL(compact_count_kernel, dim3(nb), dim3(PS_BLOCK), 0, s, mask, n, block_counts);
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(PS_BLOCK), 0, s, block_counts, (int)nb, count);
    hipLaunchKernelGGL(compact_write_kernel, dim3(nb), dim3(PS_BLOCK), 0, s, mask, n, W, block_counts, list);
    return launched();
}

}  // namespace na
