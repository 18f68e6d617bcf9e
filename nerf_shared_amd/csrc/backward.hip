// backward.hip -- training support for the fused field family: the workspace layout of a training step, and the parameter
// gradients
//   dL/draw -> the dX-chain kernel (mlp_bwd_s16.hip / mlp_bwd_split.hip: pre-activation gradients of every layer, left in
//              the workspace)
//           -> weight gradients  dW_l = g_pre(l)^T h_(l-1)   and bias gradients (column sums)
// Saved activations X and gradients G are slot-major rows [P, n] (kernels.h): bf16, or planes of fp16 hi and lo rows in split
// precision.  dW is a GEMM whose contraction runs over the points (K = hundreds of thousands) with M, N <= 256: HBM-bound
// streaming of G and X.  Every product of a model is a job of ONE launch (dw_multi_kernel / dw_multi_split_kernel; the jobs,
// their workgroup shares and their slabs are planned on the host, dw_plan.h): a job's workgroups split the points, stream
// 32-point chunks of G and X through an LDS ring with LDS-DMA, read both MFMA operands with the transposing LDS read and
// leave their [n_out x n_in] fp32 partial tiles as register dumps (slabs).  A second launch (dw_reduce_multi_kernel) sums
// each job's slabs in a fixed order and writes the nn.Linear-layout gradient, un-permuting the slot order on the way: no
// float atomics on that path, so equal inputs give equal bits.  The head of a model without view branch (output_linear)
// has fp32 FMA kernels of its own (dw_small_kernel / dw_small_split_kernel).  The generations before this one are
// described in tools/experiments/design_log_r1_r3.md.
#include <hip/hip_runtime.h>

#include "dw_plan.h"
#include "kernels.h"
#include "launch_util.h"
#include "pipeline.h"
#include "program.h"
#include "split.h"

#include <utility>

namespace na {

template <class F, int... Is>
__device__ __forceinline__ void static_for_dw_impl(F &&f, std::integer_sequence<int, Is...>) { (f(std::integral_constant<int, Is>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void static_for_dw(F &&f) { static_for_dw_impl(f, std::make_integer_sequence<int, N>{}); }

__device__ __forceinline__ int slot_to_feature(int kind, int s, int L) {
    if (kind == PERM_NAT) return s;
    const int ks = s >> 5, q = (s >> 3) & 3, j = s & 7;
    return kind == PERM_ACC ? acc16_col(ks, q, j) : gen16_col(ks, q, j, L);
}

typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

// Element e of a job's summed slabs -> its place in the nn.Linear gradients.
__device__ __forceinline__ void dw_scatter(const DwReduceArgs &a, int e, float acc) {
    if (a.inv_scale) acc *= *a.inv_scale;        // a power of two: exact
    const int n_main = a.OT * a.IT * 256;
    if (e < n_main) {
        const int r = e & 3, lane = (e >> 2) & 63, tile = e >> 8;
        const int to = tile / a.IT, ti = tile - to * a.IT;
        const int o = slot_to_feature(a.out_kind, to * 16 + 4 * (lane >> 4) + r, 0);
        const int i = slot_to_feature(a.in_kind, ti * 16 + (lane & 15), a.in_L);
        if (i >= 0 && o >= 0 && i < a.m_valid && o < a.n_valid) a.dW[(int64_t)o * a.ld_dw + a.col_off + i] = acc;
        return;
    }
    e -= n_main;
    if (e < a.OT * 16) {
        if (a.db) {
            const int o = slot_to_feature(a.out_kind, e, 0);
            if (o >= 0 && o < a.n_valid) a.db[o] = acc;
        }
        return;
    }
    e -= a.OT * 16;                      // head part: IT tiles (rows = columns of dL/draw, natural order), then 16 bias sums
    if (e < a.IT * 256) {
        const int r = e & 3, lane = (e >> 2) & 63, ti = e >> 8;
        const int row = 4 * (lane >> 4) + r - a.head_row0;
        const int i = slot_to_feature(a.in_kind, ti * 16 + (lane & 15), a.in_L);
        if (row >= 0 && row < a.head_rows && i >= 0 && i < a.m_valid) a.head_dW[(int64_t)row * a.head_ld + i] = acc;
    } else {
        const int row = e - a.IT * 256 - a.head_row0;
        if (row >= 0 && row < a.head_rows) a.head_db[row] = acc;
    }
}

// ---------------------------------------------------------------------------------------------------------
// dw2_body: a weight-gradient product as a streaming kernel that keeps HBM busy.
//   * G and X rows go straight from HBM to LDS with LDS-DMA (global_load_lds_dwordx4, no VGPR staging) into a ring of
//     four 32-point chunks, three chunks (96 KB per CU) in flight, one counted-vmcnt wait + one barrier per chunk;
//   * the LDS image is XOR-swizzled at 16-byte granularity through the DMA's per-lane SOURCE addresses (the DMA's
//     destination is lane-linear, its source is not): piece j of row r sits at j ^ swz(r), which makes the transposing
//     operand reads (ds_read_b64_tr_b16, 8 rows x 32 B per 32-lane group) conflict-free on unpadded 512-byte rows;
//   * the bias gradient (column sums of G) is one more MFMA column against an all-ones operand.
// (Reduce jobs for the previous product's slabs inside this launch do not work out: every block of a launch reserves the
// launch's 128 KB of LDS, so the ~1000 small reduce blocks would each occupy a whole CU.)
// ---------------------------------------------------------------------------------------------------------
// One 32-lane group of a transposing read covers rows {0..3, 8..11} (+4 for the second half) x 32 bytes.  Rows of >= 256
// bytes all start at bank 0, so the eight rows need eight different piece pairs: XOR with 0, 2, .., 14.  Rows of 128 bytes
// (PIECES == 8) alternate between the two halves of the banks, so the four even rows {0, 2, 8, 10} (and the four odd ones)
// need four different pairs: XOR with 0, 2, 4, 6.  Both forms satisfy swz(r + 4) == swz(r).
#ifdef NERF_AMD_X_DW_STAMPS
// tools/micro/dw_stamps.py: when each workgroup of the last dw_multi_kernel launch started and ended (100 MHz clock)
__device__ unsigned long long g_dw_stamps[4 * 512];
extern "C" int nerf_amd_x_dw_stamps(unsigned long long *out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dw_stamps), sizeof(g_dw_stamps)) == hipSuccess ? 0 : -1;
}
#endif

template <int PIECES>
__device__ __forceinline__ int dw_swz(int r) {
    static_assert(PIECES == 4 || PIECES == 8 || (PIECES >= 16 && (PIECES & (PIECES - 1)) == 0), "unsupported row width");
    // 64-byte rows (PIECES == 4): four rows span the banks once, so rows {0..3} never collide and rows {8..11} take the
    // other piece pair
    if (PIECES == 4) return 2 * ((r >> 3) & 1);
    if (PIECES == 8) return 2 * (((r >> 1) & 1) | (((r >> 3) & 1) << 1));
    return 2 * ((r & 3) | (((r >> 3) & 1) << 2));
}

template <int PIECES>
__device__ __forceinline__ bf16x8 tr_frag_swz(uint32_t img, int col0, int lane) {
    // 8 consecutive image rows (points 8g..8g+7) of column col0 + (lane & 15), as an MFMA 16x16x32 operand, from the
    // swizzled image: 16-byte piece pc of row r lives at piece position pc ^ dw_swz(r).
    constexpr int row_bytes = PIECES * 16;
    const int i = lane & 15, g = lane >> 4;
    const int r = 8 * g + (i >> 2);
    const int pc = (col0 >> 3) + ((i & 3) >> 1);
    const uint32_t p = img + r * row_bytes + ((pc ^ dw_swz<PIECES>(r)) << 4) + ((i & 1) << 3);
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(uintptr_t)(p));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(uintptr_t)(p + 4 * row_bytes));
    typedef __attribute__((ext_vector_type(8))) short s16x8;
    const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
}

// One 1-KiB LDS-DMA piece: lane l fetches 16 bytes from g (per lane) into lds_base + 16 l.
__device__ __forceinline__ void dma_piece(const char *g, uint32_t lds_base) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\t" "s_mov_b32 m0, %2\n\t" "s_nop 0\n\t" "global_load_lds_dwordx4 %1, off\n\t" "s_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(g), "s"(lds_base) : "memory");
}

// HEAD: a head product (alpha_linear / rgb_linear: G = columns of dL/draw) rides on this job -- same X, one more 16-row
// A operand per chunk.  Its operand needs no transposing read: the dX-chain kernel left dL/draw transposed inside 32-point
// chunks (kernels.h g_rawt), 16 bytes per (point group, column) = one lane's MFMA A operand, so wave 0 moves the chunk's
// 256 bytes into the ring slot with one more LDS-DMA instruction (lanes whose row is not a column of dL/draw fetch a valid
// 16 bytes too and are zeroed after the LDS read) and every wave reads its operand back with one ds_read_b128.  The 16
// head x X tiles are dealt two to a wave.
template <int OT, int IT, int WO, int WI, bool HEAD = false>
__device__ __forceinline__ void dw2_body(const DwArgs &a, const int wg, const int nwg) {
    static_assert(WO * WI == 8 && OT % WO == 0 && IT % WI == 0 && OT >= 4 && IT >= 2, "bad shape");
    constexpr int TO = OT / WO, TI = IT / WI;
    static_assert(!HEAD || TI == 2 * WO, "the head's X tiles are dealt two to a wave");
    constexpr int RG = OT * 32, RX = IT * 32;                   // row bytes (unpadded)
    constexpr int PG = OT * 2, PX = IT * 2;                     // 16-byte pieces per row
    constexpr int IMG_GX = 32 * (RG + RX);                      // G and X rows of one chunk
    constexpr int IMG = IMG_GX + (HEAD ? 1024 : 0);             // one chunk's image (+ the head operand)
    constexpr int NI = OT + IT, CNT = (NI + 7) / 8;             // 1-KiB DMA instructions per chunk; per wave at most
    constexpr int REM = NI - 8 * (CNT - 1);                     // waves below REM issue CNT per chunk, the others CNT - 1
    // ring slots: what fits in 128 KiB, at least 4 and at most 12 -- a narrow product keeps as many BYTES in flight as a
    // wide one (a workgroup's rate is bytes in flight / latency, and the one-launch path shares the CUs by bytes)
    constexpr int NS = DW2_NS(OT, IT);
    static_assert((NS - 2) * (CNT + (HEAD ? 1 : 0)) <= 63, "vmcnt field is 6 bits");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wo = wave / WI, wi = wave % WI;
    const uint32_t ring = (uint32_t)(uintptr_t)smem;

    const int64_t n_chunks = (a.P + 31) / 32;
    const int64_t first = wg, stride = nwg;
    const int64_t n_local = wg < n_chunks ? (n_chunks - wg + nwg - 1) / nwg : 0;     // chunks wg, wg + nwg, ...
    // this wave's DMA instructions of a chunk: j = wave, wave + 8, ... below NI -- CNT of them, or CNT - 1 for the waves
    // from REM on (a count per wave, uniform inside it, so the counted waits stay compile-time constants: wait_chunk below)
    const bool full = REM == 8 || wave < REM;
    auto issue_chunk = [&](int64_t i) {
        int64_t ch = first + i * stride;
        if (ch >= n_chunks) ch = n_chunks - 1;                  // past the end: a harmless re-read that is never consumed
        const uint32_t slot = ring + (uint32_t)(i % NS) * IMG;
        const int64_t p0 = ch * 32;
#pragma unroll
        for (int k = 0; k < CNT; ++k) {
            const int j = wave + 8 * k;
            if (k == CNT - 1 && !full) break;
            const bool is_g = j < OT;
            const int jj = is_g ? j : j - OT;
            const int e = 64 * jj + lane;                       // 16-byte piece of the G (or X) image
            const int pr = is_g ? PG : PX;
            const int r = e / pr, pos = e % pr;
            int64_t p = p0 + r;
            if (p >= pad_points(a.P)) p = pad_points(a.P) - 1;  // rows exist up to the padded point count (kernels.h)
            const char *src = is_g ? reinterpret_cast<const char *>(a.G) + (p * a.ldg) * 2 : reinterpret_cast<const char *>(a.X) + (p * a.ldx) * 2;
            src += (pos ^ (is_g ? dw_swz<PG>(r) : dw_swz<PX>(r))) << 4;
            dma_piece(src, slot + (is_g ? 0 : 32 * RG) + 1024 * jj);
        }
        if constexpr (HEAD) {
            if (wave == 0)                                      // the chunk's head operand: lane (i, g) <- 16 bytes of (group g, column i & 3)
                dma_piece(reinterpret_cast<const char *>(a.H) + ch * 256 + ((lane >> 4) * 4 + (lane & 3)) * 16, slot + IMG_GX);
        }
    };

    f32x4 acc[TO][TI], accb[TO];
    f32x4 acch[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, acchb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int x = 0; x < TO; ++x) {
        accb[x] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int y = 0; y < TI; ++y) acc[x][y] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    bf16x8 ones;
#pragma unroll
    for (int j = 0; j < 8; ++j) ones[j] = (__bf16)1.0f;

    if (n_local > 0) {
#pragma unroll
        for (int i = 0; i < NS - 1; ++i) issue_chunk(i);
        for (int64_t i = 0; i < n_local; ++i) {
            // chunk i has landed (this wave's pieces; chunks i+1, i+2 stay in flight), everyone agrees, then the slot of
            // chunk i-1 -- which every wave finished reading before it came here -- is refilled with chunk i+3
            if (HEAD && wave == 0) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((NS - 2) * (CNT + 1)) : "memory");   // wave 0 issues one more piece per chunk
            else if (full) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((NS - 2) * CNT) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((NS - 2) * (CNT - 1)) : "memory");
#ifdef NERF_AMD_X_DW_STAMPS
            if (tid == 0 && (i == 0 || i == n_local / 2)) {         // first chunk landed | half way: packed into one word
                const unsigned long long t = wall_clock64() - g_dw_stamps[4 * blockIdx.x];
                if (i == 0) g_dw_stamps[4 * blockIdx.x + 3] = t; else g_dw_stamps[4 * blockIdx.x + 3] |= t << 32;
            }
#endif
            issue_chunk(i + NS - 1);
            const uint32_t gimg = ring + (uint32_t)(i % NS) * IMG, ximg = gimg + 32 * RG;
            const int64_t ch = first + i * stride;
            if (ch == n_chunks - 1 && (a.P & 31)) {             // the last chunk: rows past P hold the padding points' data
                const int first = (int)(a.P & 31);
                for (int e = tid; e < (32 - first) * (RG + RX) / 16; e += 512) {
                    const int gp = (32 - first) * PG;
                    const uint32_t off = e < gp ? gimg + first * RG + e * 16 : ximg + first * RX + (e - gp) * 16;
                    *(__attribute__((address_space(3))) u32x4 *)(uintptr_t)off = (u32x4){0u, 0u, 0u, 0u};
                }
                __syncthreads();
            }
            bf16x8 A[TO], B[TI];
#pragma unroll
            for (int x = 0; x < TO; ++x) A[x] = tr_frag_swz<PG>(gimg, (wo * TO + x) * 16, lane);
#pragma unroll
            for (int y = 0; y < TI; ++y) B[y] = tr_frag_swz<PX>(ximg, (wi * TI + y) * 16, lane);
#pragma unroll
            for (int x = 0; x < TO; ++x) {
#pragma unroll
                for (int y = 0; y < TI; ++y)
                    acc[x][y] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[x], B[y], acc[x][y], 0, 0, 0);
                if (wi == 0) accb[x] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[x], ones, accb[x], 0, 0, 0);
            }
            if constexpr (HEAD) {
                typedef __attribute__((address_space(3))) const bf16x8 lds_bf16x8;
                bf16x8 Ah = *(lds_bf16x8 *)(uintptr_t)(gimg + IMG_GX + lane * 16);
                if ((lane & 15) >= 4) Ah = bf16x8{};            // rows 4..15 of the head tile do not exist
                static_for_dw<WO>([&](auto x_) {                // this wave's two X tiles: 2 wo, 2 wo + 1 of its TI
                    constexpr int x = x_;
                    if (wo == x) {
                        acch[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, B[2 * x], acch[0], 0, 0, 0);
                        acch[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, B[2 * x + 1], acch[1], 0, 0, 0);
                    }
                });
                if (wave == 0) acchb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, ones, acchb, 0, 0, 0);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the trailing re-reads: no DMA may outlive the workgroup
    }
    // ---- this workgroup's partial tile as a register dump (1 KiB per 16x16 tile, fully coalesced) + the bias partials
    float *slab = a.slab + (int64_t)wg * dw_slab_floats(OT, IT, HEAD ? 1 : 0);
#pragma unroll
    for (int x = 0; x < TO; ++x)
#pragma unroll
        for (int y = 0; y < TI; ++y)
            *reinterpret_cast<f32x4 *>(slab + (((wo * TO + x) * IT + (wi * TI + y)) * 64 + lane) * 4) = acc[x][y];
    if (wi == 0 && (lane & 15) == 0) {                          // every column of accb holds the same sums: take column 0
#pragma unroll
        for (int x = 0; x < TO; ++x)
            *reinterpret_cast<f32x4 *>(slab + OT * IT * 256 + (wo * TO + x) * 16 + 4 * (lane >> 4)) = accb[x];
    }
    if constexpr (HEAD) {                                       // head tiles behind the main part: [IT][64 lanes][4], then 16 bias sums
        float *hs = slab + OT * IT * 256 + OT * 16;
#pragma unroll
        for (int t = 0; t < 2; ++t)
            *reinterpret_cast<f32x4 *>(hs + ((wi * TI + 2 * wo + t) * 64 + lane) * 4) = acch[t];
        if (wave == 0 && (lane & 15) == 0) *reinterpret_cast<f32x4 *>(hs + IT * 256 + 4 * (lane >> 4)) = acchb;
    }
}

// A head product alone (rgb_linear: nothing else multiplies the view layer's output): X rows only in the ring, the head
// operand as in dw2_body, one X tile per wave.
template <int IT>
__device__ __forceinline__ void dw_head_body(const DwArgs &a, const int wg, const int nwg) {
    static_assert(IT == 8, "one 16-column X tile per wave");
    constexpr int RX = IT * 32, PX = IT * 2, IMG_X = 32 * RX, IMG = IMG_X + 1024;
    constexpr int NS = 12;                                      // 12 x 9 KiB: as many bytes in flight as a wide product keeps
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t ring = (uint32_t)(uintptr_t)smem;
    const int64_t n_chunks = (a.P + 31) / 32;
    const int64_t n_local = wg < n_chunks ? (n_chunks - wg + nwg - 1) / nwg : 0;
    auto issue_chunk = [&](int64_t i) {
        int64_t ch = wg + i * nwg;
        if (ch >= n_chunks) ch = n_chunks - 1;                  // past the end: a harmless re-read that is never consumed
        const uint32_t slot = ring + (uint32_t)(i % NS) * IMG;
        const int e = 64 * wave + lane;                         // 16-byte piece of the X image: this wave's 1 KiB
        const int r = e / PX, pos = e % PX;
        int64_t p = ch * 32 + r;
        if (p >= pad_points(a.P)) p = pad_points(a.P) - 1;
        dma_piece(reinterpret_cast<const char *>(a.X) + (p * a.ldx) * 2 + ((pos ^ dw_swz<PX>(r)) << 4), slot + 1024 * wave);
        if (wave == 0)
            dma_piece(reinterpret_cast<const char *>(a.H) + ch * 256 + ((lane >> 4) * 4 + (lane & 3)) * 16, slot + IMG_X);
    };
    f32x4 acc = {0.f, 0.f, 0.f, 0.f}, accb = {0.f, 0.f, 0.f, 0.f};
    bf16x8 ones;
#pragma unroll
    for (int j = 0; j < 8; ++j) ones[j] = (__bf16)1.0f;
    if (n_local > 0) {
#pragma unroll
        for (int i = 0; i < NS - 1; ++i) issue_chunk(i);
        for (int64_t i = 0; i < n_local; ++i) {
            if (wave == 0) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((NS - 2) * 2) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(NS - 2) : "memory");
            issue_chunk(i + NS - 1);
            const uint32_t ximg = ring + (uint32_t)(i % NS) * IMG;
            typedef __attribute__((address_space(3))) const bf16x8 lds_bf16x8;
            bf16x8 Ah = *(lds_bf16x8 *)(uintptr_t)(ximg + IMG_X + lane * 16);
            if ((lane & 15) >= 4) Ah = bf16x8{};
            // rows past P of the last chunk hold the padding points' saved activations: finite, and their dL/draw is zero
            const bf16x8 B = tr_frag_swz<PX>(ximg, wave * 16, lane);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, B, acc, 0, 0, 0);
            if (wave == 0) accb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah, ones, accb, 0, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    float *slab = a.slab + (int64_t)wg * dw_slab_floats(0, IT, 1);
    *reinterpret_cast<f32x4 *>(slab + (wave * 64 + lane) * 4) = acc;
    if (wave == 0 && (lane & 15) == 0) *reinterpret_cast<f32x4 *>(slab + IT * 256 + 4 * (lane >> 4)) = accb;
}


// ---------------------------------------------------------------------------------------------------------
// Split-precision weight gradients (NERF_AMD_PREC_FP32_SPLIT, split.h): G and X arrive as planes of fp16 hi rows and fp16
// lo rows (lo = residual x 2^11), exactly as the training forward and the dX chain hold them.  dW = G^T X keeps ONE
// accumulator per tile:
//     acc += G_hi X_hi  +  (2^-11 G_hi) X_lo  +  G_lo (2^-11 X_hi)
// where the two rescaled hi operands are made in registers (one packed fp16 multiply per register; where that product
// falls below fp16's normal range it loses bits of a term that is itself 2^-11 of the sum -- measured on the CPU before
// this was written, tools/experiments/split_bwd_sim.py "dW sym": 1e-6 of fp32 autograd at the loss scale split.h picks,
// 1.6e-4 even when it is 2^14 off).  Bias gradients: G_hi . 1 + G_lo . 2^-11.  The chunk image is twice the bf16 one
// (64 KiB for a 256 x 256 product), so the ring holds two chunks: one in flight while one is consumed.
// ---------------------------------------------------------------------------------------------------------
#define MFMA_F16(a_, b_, c_) __builtin_amdgcn_mfma_f32_16x16x32_f16(a_, b_, c_, 0, 0, 0)

template <int OT, int IT, int WO, int WI, bool HEAD = false>
__device__ __forceinline__ void dw2s_body(const DwArgs &a, const int wg, const int nwg) {
    static_assert(WO * WI == 8 && OT % WO == 0 && IT % WI == 0 && OT >= 4 && IT >= 2, "bad shape");
    constexpr int TO = OT / WO, TI = IT / WI;
    static_assert(!HEAD || TI == 2 * WO, "the head's X tiles are dealt two to a wave");
    constexpr int RG = OT * 32, RX = IT * 32;                   // row bytes of one plane (unpadded)
    constexpr int PG = OT * 2, PX = IT * 2;                     // 16-byte pieces per row
    constexpr int IMG_G = 32 * RG, IMG_X = 32 * RX;             // one plane of one chunk
    constexpr int IMG_GX = 2 * (IMG_G + IMG_X);                 // G_hi, G_lo, X_hi, X_lo
    constexpr int IMG = IMG_GX + (HEAD ? 2048 : 0);             // + the head operand's two planes
    constexpr int NI = 2 * (OT + IT), CNT = (NI + 7) / 8;       // 1-KiB DMA instructions per chunk; per wave at most
    constexpr int REM = NI - 8 * (CNT - 1);                     // waves below REM issue CNT per chunk, the others CNT - 1
    constexpr int NS = DW2S_NS(OT, IT);
    static_assert((NS - 2) * (CNT + (HEAD ? 2 : 0)) <= 63, "vmcnt field is 6 bits");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wo = wave / WI, wi = wave % WI;
    const uint32_t ring = (uint32_t)(uintptr_t)smem;

    const int64_t n_chunks = (a.P + 31) / 32;
    const int64_t n_local = wg < n_chunks ? (n_chunks - wg + nwg - 1) / nwg : 0;     // chunks wg, wg + nwg, ...
    // The ring DMA as buffer_load ... lds: a buffer resource per plane (scalar), ONE per-lane 32-bit offset per piece that
    // does not depend on the chunk (row inside the chunk x row bytes + swizzled position), the chunk as the scalar offset --
    // no 64-bit per-lane address arithmetic inside the loop, and rows past the arrays' end read as zero instead of needing a
    // clamp.  This wave's pieces of a chunk: j = wave, wave + 8, ... below NI of the pieces G_hi | G_lo | X_hi | X_lo: CNT of
    // them, or CNT - 1 for the waves from REM on (uniform per wave, so the counted waits stay compile-time constants).
    const bool full = REM == 8 || wave < REM;
    typedef __attribute__((ext_vector_type(4))) unsigned rsrc_t;
    const unsigned g_bytes = (unsigned)(pad_points(a.P) * a.ldg * 2), x_bytes = (unsigned)(pad_points(a.P) * a.ldx * 2);
    const rsrc_t rs_plane[4] = {make_rsrc(a.G, g_bytes), make_rsrc(a.G_lo, g_bytes), make_rsrc(a.X, x_bytes), make_rsrc(a.X_lo, x_bytes)};
    unsigned voff[CNT], lds_off[CNT];
    int plane[CNT];
#pragma unroll
    for (int k = 0; k < CNT; ++k) {
        int j = wave + 8 * k;
        if (j >= NI) j = NI - 1;
        const bool is_g = j < 2 * OT;
        const int jp = is_g ? j : j - 2 * OT;                   // piece inside the two planes of G (or of X)
        const int n_pl = is_g ? OT : IT;                        // pieces per plane
        const bool lo = jp >= n_pl;
        const int jj = lo ? jp - n_pl : jp;
        const int e = 64 * jj + lane;                           // 16-byte piece of the plane's image
        const int rg = e / PG, posg = e % PG, rx = e / PX, posx = e % PX;
        const unsigned vg = (unsigned)(rg * a.ldg * 2 + ((posg ^ dw_swz<PG>(rg)) << 4));
        const unsigned vx = (unsigned)(rx * a.ldx * 2 + ((posx ^ dw_swz<PX>(rx)) << 4));
        voff[k] = is_g ? vg : vx;
        lds_off[k] = __builtin_amdgcn_readfirstlane((is_g ? 0 : 2 * IMG_G) + (lo ? (is_g ? IMG_G : IMG_X) : 0) + 1024 * jj);
        plane[k] = __builtin_amdgcn_readfirstlane((is_g ? 0 : 2) + (lo ? 1 : 0));
    }
    rsrc_t rs_head[2];
    unsigned voff_head = 0;
    if constexpr (HEAD) {
        rs_head[0] = make_rsrc(a.H, (unsigned)(n_chunks * 256));
        rs_head[1] = make_rsrc(a.H_lo, (unsigned)(n_chunks * 256));
        voff_head = ((lane >> 4) * 4 + (lane & 3)) * 16;        // lane (i, g) <- 16 bytes of (group g, column i & 3)
    }
    auto dma_buf = [&](unsigned vo, const rsrc_t &rs, unsigned so, uint32_t lds_base) {
        unsigned keep;
        asm volatile("s_mov_b32 %0, m0\n\t" "s_mov_b32 m0, %3\n\t" "s_nop 0\n\t" "buffer_load_dwordx4 %1, %2, %4 offen lds\n\t" "s_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(vo), "s"(rs), "s"(lds_base), "s"(so) : "memory");
    };
    auto issue_chunk = [&](int64_t i) {
        int64_t ch = wg + i * nwg;
        if (ch >= n_chunks) ch = n_chunks - 1;                  // past the end: a harmless re-read that is never consumed
        const uint32_t slot = ring + (uint32_t)(i % NS) * IMG;
        const unsigned so_g = __builtin_amdgcn_readfirstlane((unsigned)(ch * 32 * a.ldg * 2));
        const unsigned so_x = __builtin_amdgcn_readfirstlane((unsigned)(ch * 32 * a.ldx * 2));
#pragma unroll
        for (int k = 0; k < CNT; ++k) {
            if (k == CNT - 1 && !full) break;
            const int pl = plane[k];
            const rsrc_t rs = pl == 0 ? rs_plane[0] : pl == 1 ? rs_plane[1] : pl == 2 ? rs_plane[2] : rs_plane[3];
            dma_buf(voff[k], rs, pl < 2 ? so_g : so_x, __builtin_amdgcn_readfirstlane(slot + lds_off[k]));
        }
        if constexpr (HEAD) {
            if (wave == 0) {                                    // the chunk's head operand, both planes
                const unsigned so_h = __builtin_amdgcn_readfirstlane((unsigned)(ch * 256));
                dma_buf(voff_head, rs_head[0], so_h, __builtin_amdgcn_readfirstlane(slot + IMG_GX));
                dma_buf(voff_head, rs_head[1], so_h, __builtin_amdgcn_readfirstlane(slot + IMG_GX + 1024));
            }
        }
    };

    f32x4 acc[TO][TI], accb[TO];
    f32x4 acch[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, acchb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int x = 0; x < TO; ++x) {
        accb[x] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int y = 0; y < TI; ++y) acc[x][y] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    f16x8 ones, ones_s;
#pragma unroll
    for (int j = 0; j < 8; ++j) { ones[j] = (_Float16)1.0f; ones_s[j] = (_Float16)SPLIT_INV; }
    const _Float16 kinv = (_Float16)SPLIT_INV;
    using PGc = std::integral_constant<int, PG>;
    using PXc = std::integral_constant<int, PX>;

    if (n_local > 0) {
#pragma unroll
        for (int i = 0; i < NS - 1; ++i) issue_chunk(i);
        for (int64_t i = 0; i < n_local; ++i) {
            // chunk i has landed (this wave's pieces; younger chunks stay in flight), everyone agrees, then the slot of
            // chunk i-1 -- which every wave finished reading before it came here -- is refilled with chunk i+NS-1
            if (HEAD && wave == 0) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((NS - 2) * (CNT + 2)) : "memory");
            else if (full) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((NS - 2) * CNT) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((NS - 2) * (CNT - 1)) : "memory");
            issue_chunk(i + NS - 1);
            const uint32_t g_hi = ring + (uint32_t)(i % NS) * IMG, g_lo = g_hi + IMG_G, x_hi = g_hi + 2 * IMG_G, x_lo = x_hi + IMG_X;
            const int64_t ch = wg + i * nwg;
            if (ch == n_chunks - 1 && (a.P & 31)) {             // the last chunk: rows past P hold the padding points' data
                const int first = (int)(a.P & 31);
                const int per_g = (32 - first) * PG, per_x = (32 - first) * PX;     // 16-byte pieces to clear per plane
                for (int e = tid; e < 2 * (per_g + per_x); e += 512) {
                    uint32_t off;
                    if (e < per_g) off = g_hi + first * RG + e * 16;
                    else if (e < 2 * per_g) off = g_lo + first * RG + (e - per_g) * 16;
                    else if (e < 2 * per_g + per_x) off = x_hi + first * RX + (e - 2 * per_g) * 16;
                    else off = x_lo + first * RX + (e - 2 * per_g - per_x) * 16;
                    *(__attribute__((address_space(3))) u32x4 *)(uintptr_t)off = (u32x4){0u, 0u, 0u, 0u};
                }
                __syncthreads();
            }
            // (an opaque copy of the lane id per chunk: otherwise the 24 swizzled operand addresses of the body are loop
            // invariants, get hoisted and spill)
            int lane_o = lane;
            asm volatile("" : "+v"(lane_o));
            auto frag = [&](auto pieces_, uint32_t img, int col0) {
                return __builtin_bit_cast(f16x8, tr_frag_swz<decltype(pieces_)::value>(img, col0, lane_o));
            };
            f16x8 A[TO], Ah = {}, Ahs = {}, Al_h = {};
            if constexpr (HEAD) {
                typedef __attribute__((address_space(3))) const f16x8 lds_f16x8;
                Ah = *(lds_f16x8 *)(uintptr_t)(g_hi + IMG_GX + lane * 16);
                Al_h = *(lds_f16x8 *)(uintptr_t)(g_hi + IMG_GX + 1024 + lane * 16);
                if ((lane & 15) >= 4) { Ah = f16x8{}; Al_h = f16x8{}; }     // rows 4..15 of the head tile do not exist
                Ahs = Ah * kinv;
            }
            // Only the G-side operands stay in registers; the X-side fragments are re-read from LDS for every term (three
            // transposing reads per X tile and chunk instead of two: LDS has the bandwidth, the register file has no room
            // for TI more fragments beside the TO x TI accumulators).  Straight-line code: every wave computes the bias
            // column and the head's bias column (only the waves that own them write them out).
            // ---- hi x hi
#pragma unroll
            for (int x = 0; x < TO; ++x) {
                A[x] = frag(PGc{}, g_hi, (wo * TO + x) * 16);
                accb[x] = MFMA_F16(A[x], ones, accb[x]);
            }
            static_for_dw<TI>([&](auto y_) {
                constexpr int y = y_;
                const f16x8 bh = frag(PXc{}, x_hi, (wi * TI + y) * 16);
#pragma unroll
                for (int x = 0; x < TO; ++x) acc[x][y] = MFMA_F16(A[x], bh, acc[x][y]);
            });
            // ---- (2^-11 G_hi) x X_lo
#pragma unroll
            for (int x = 0; x < TO; ++x) A[x] = A[x] * kinv;
            static_for_dw<TI>([&](auto y_) {
                constexpr int y = y_;
                const f16x8 bl = frag(PXc{}, x_lo, (wi * TI + y) * 16);
#pragma unroll
                for (int x = 0; x < TO; ++x) acc[x][y] = MFMA_F16(A[x], bl, acc[x][y]);
            });
            // ---- G_lo x (2^-11 X_hi)
#pragma unroll
            for (int x = 0; x < TO; ++x) {
                A[x] = frag(PGc{}, g_lo, (wo * TO + x) * 16);
                accb[x] = MFMA_F16(A[x], ones_s, accb[x]);
            }
            static_for_dw<TI>([&](auto y_) {
                constexpr int y = y_;
                const f16x8 bs = frag(PXc{}, x_hi, (wi * TI + y) * 16) * kinv;
#pragma unroll
                for (int x = 0; x < TO; ++x) acc[x][y] = MFMA_F16(A[x], bs, acc[x][y]);
            });
            if constexpr (HEAD) {                               // this wave's two X tiles of the head product: 2 wo, 2 wo + 1 of its TI
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int col = (wi * TI + 2 * wo + t) * 16;
                    const f16x8 bh = frag(PXc{}, x_hi, col), bl = frag(PXc{}, x_lo, col);
                    acch[t] = MFMA_F16(Ah, bh, acch[t]);
                    acch[t] = MFMA_F16(Ahs, bl, acch[t]);
                    acch[t] = MFMA_F16(Al_h, bh * kinv, acch[t]);
                }
                acchb = MFMA_F16(Ah, ones, acchb);
                acchb = MFMA_F16(Al_h, ones_s, acchb);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the trailing re-reads: no DMA may outlive the workgroup
    }
    // ---- this workgroup's partial tile as a register dump, laid out exactly like dw2_body's
    float *slab = a.slab + (int64_t)wg * dw_slab_floats(OT, IT, HEAD ? 1 : 0);
#pragma unroll
    for (int x = 0; x < TO; ++x)
#pragma unroll
        for (int y = 0; y < TI; ++y)
            *reinterpret_cast<f32x4 *>(slab + (((wo * TO + x) * IT + (wi * TI + y)) * 64 + lane) * 4) = acc[x][y];
    if (wi == 0 && (lane & 15) == 0) {
#pragma unroll
        for (int x = 0; x < TO; ++x)
            *reinterpret_cast<f32x4 *>(slab + OT * IT * 256 + (wo * TO + x) * 16 + 4 * (lane >> 4)) = accb[x];
    }
    if constexpr (HEAD) {
        float *hs = slab + OT * IT * 256 + OT * 16;
#pragma unroll
        for (int t = 0; t < 2; ++t)
            *reinterpret_cast<f32x4 *>(hs + ((wi * TI + 2 * wo + t) * 64 + lane) * 4) = acch[t];
        if (wave == 0 && (lane & 15) == 0) *reinterpret_cast<f32x4 *>(hs + IT * 256 + 4 * (lane >> 4)) = acchb;
    }
}

// A head product alone in split precision (rgb_linear): the two planes of X rows + the head operand's two planes.
template <int IT>
__device__ __forceinline__ void dw_head_split_body(const DwArgs &a, const int wg, const int nwg) {
    static_assert(IT == 8, "one 16-column X tile per wave");
    constexpr int RX = IT * 32, PX = IT * 2, IMG_X = 32 * RX, IMG = 2 * IMG_X + 2048;
    constexpr int NS = 7;                                       // 7 x 18 KiB
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t ring = (uint32_t)(uintptr_t)smem;
    const int64_t n_chunks = (a.P + 31) / 32;
    const int64_t n_local = wg < n_chunks ? (n_chunks - wg + nwg - 1) / nwg : 0;
    auto issue_chunk = [&](int64_t i) {
        int64_t ch = wg + i * nwg;
        if (ch >= n_chunks) ch = n_chunks - 1;
        const uint32_t slot = ring + (uint32_t)(i % NS) * IMG;
        const int e = 64 * wave + lane;                         // 16-byte piece of a plane's X image: this wave's 1 KiB
        const int r = e / PX, pos = e % PX;
        int64_t p = ch * 32 + r;
        if (p >= pad_points(a.P)) p = pad_points(a.P) - 1;
        const int64_t off = (p * a.ldx) * 2 + ((pos ^ dw_swz<PX>(r)) << 4);
        dma_piece(reinterpret_cast<const char *>(a.X) + off, slot + 1024 * wave);
        dma_piece(reinterpret_cast<const char *>(a.X_lo) + off, slot + IMG_X + 1024 * wave);
        if (wave == 0) {
            const int64_t ho = ch * 256 + ((lane >> 4) * 4 + (lane & 3)) * 16;
            dma_piece(reinterpret_cast<const char *>(a.H) + ho, slot + 2 * IMG_X);
            dma_piece(reinterpret_cast<const char *>(a.H_lo) + ho, slot + 2 * IMG_X + 1024);
        }
    };
    f32x4 acc = {0.f, 0.f, 0.f, 0.f}, accb = {0.f, 0.f, 0.f, 0.f};
    f16x8 ones, ones_s;
#pragma unroll
    for (int j = 0; j < 8; ++j) { ones[j] = (_Float16)1.0f; ones_s[j] = (_Float16)SPLIT_INV; }
    const _Float16 kinv = (_Float16)SPLIT_INV;
    if (n_local > 0) {
#pragma unroll
        for (int i = 0; i < NS - 1; ++i) issue_chunk(i);
        for (int64_t i = 0; i < n_local; ++i) {
            if (wave == 0) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((NS - 2) * 4) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((NS - 2) * 2) : "memory");
            issue_chunk(i + NS - 1);
            const uint32_t x_hi = ring + (uint32_t)(i % NS) * IMG, x_lo = x_hi + IMG_X;
            typedef __attribute__((address_space(3))) const f16x8 lds_f16x8;
            f16x8 Ah = *(lds_f16x8 *)(uintptr_t)(x_hi + 2 * IMG_X + lane * 16);
            f16x8 Al = *(lds_f16x8 *)(uintptr_t)(x_hi + 2 * IMG_X + 1024 + lane * 16);
            if ((lane & 15) >= 4) { Ah = f16x8{}; Al = f16x8{}; }
            // rows past P of the last chunk hold the padding points' saved activations: finite, and their dL/draw is zero
            const f16x8 Bh = __builtin_bit_cast(f16x8, tr_frag_swz<PX>(x_hi, wave * 16, lane));
            const f16x8 Bl = __builtin_bit_cast(f16x8, tr_frag_swz<PX>(x_lo, wave * 16, lane));
            acc = MFMA_F16(Ah, Bh, acc);
            acc = MFMA_F16(Ah * kinv, Bl, acc);
            acc = MFMA_F16(Al, Bh * kinv, acc);
            if (wave == 0) { accb = MFMA_F16(Ah, ones, accb); accb = MFMA_F16(Al, ones_s, accb); }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    float *slab = a.slab + (int64_t)wg * dw_slab_floats(0, IT, 1);
    *reinterpret_cast<f32x4 *>(slab + (wave * 64 + lane) * 4) = acc;
    if (wave == 0 && (lane & 15) == 0) *reinterpret_cast<f32x4 *>(slab + IT * 256 + 4 * (lane >> 4)) = accb;
}

// The head of a model without view branch (output_linear): G = NO <= 4 natural-order columns of g_rawb [P, 16], X = [P, n_in]
// slot-major.  A block walks 256-row tiles; a thread owns 8 consecutive X columns (one 16-byte load
// per row) of every (256 / groups)-th row.  Partial sums meet in LDS and leave as one slab row per
// block ([NO][n_in] weights, then NO biases); dw_small_reduce_kernel sums the rows.
template <int NO>
__device__ __forceinline__ void dw_small_body(const uint16_t *G, int ldg, int g_col0, const uint16_t *X, int ldx, int n_in, int64_t P,
                                              float *slab, float (*red)[256 + 1] /* LDS [NO][257] */, const int wg, const int nwg) {
    const int groups = n_in / 8;                       // column groups per row (32 for 256 columns, 16 for 128)
    const int rows_par = 256 / groups;                 // rows in flight per block
    const int cg = threadIdx.x % groups, ty = threadIdx.x / groups;
    float acc[NO][8], bs[NO];
#pragma unroll
    for (int k = 0; k < NO; ++k) {
        bs[k] = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[k][j] = 0.f;
    }
    for (int64_t r0 = (int64_t)wg * 256; r0 < P; r0 += (int64_t)nwg * 256) {
        const int64_t r1 = r0 + 256 < P ? r0 + 256 : P;
#pragma unroll 4
        for (int64_t p = r0 + ty; p < r1; p += rows_par) {
            const u32x4 xv = *reinterpret_cast<const u32x4 *>(X + p * ldx + cg * 8);
            float x[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                x[2 * j] = __builtin_bit_cast(float, xv[j] << 16);
                x[2 * j + 1] = __builtin_bit_cast(float, xv[j] & 0xffff0000u);
            }
            // the row's four gradient values (the aligned group of four columns g_col0 lies in) as one 8-byte load
            typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
            const u32x2 gv = *reinterpret_cast<const u32x2 *>(G + p * ldg + (g_col0 & ~3));
#pragma unroll
            for (int k = 0; k < NO; ++k) {
                const int col = (g_col0 & 3) + k;
                const unsigned word = (col & 2) ? gv[1] : gv[0];
                const float g = __builtin_bit_cast(float, (col & 1) ? (word & 0xffff0000u) : (word << 16));
                if (cg == 0) bs[k] += g;
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[k][j] += g * x[j];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NO; ++k)
        if (threadIdx.x < 256) red[k][threadIdx.x] = 0.f;
    if (threadIdx.x < NO) red[threadIdx.x][256] = 0.f;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NO; ++k) {
#pragma unroll
        for (int j = 0; j < 8; ++j) atomicAdd(&red[k][cg * 8 + j], acc[k][j]);
        if (cg == 0) atomicAdd(&red[k][256], bs[k]);
    }
    __syncthreads();
    float *row = slab + (int64_t)wg * (NO * n_in + NO);
    if ((int)threadIdx.x < n_in)
#pragma unroll
        for (int k = 0; k < NO; ++k) row[k * n_in + threadIdx.x] = red[k][threadIdx.x];
    if (threadIdx.x < NO) row[NO * n_in + threadIdx.x] = red[threadIdx.x][256];
}

template <int NO>
__global__ __launch_bounds__(256) void dw_small_kernel(const uint16_t *G, int ldg, int g_col0, const uint16_t *X, int ldx, int n_in,
                                                       int64_t P, float *slab) {
    __shared__ float red[NO][256 + 1];
    dw_small_body<NO>(G, ldg, g_col0, X, ldx, n_in, P, slab, red, blockIdx.x, gridDim.x);
}

// dW[k][feature(slot)] / db[k] = sum of the slab rows dw_small_kernel left; 64 elements per block.
__global__ __launch_bounds__(1024) void dw_small_reduce_kernel(const float *slab, int n_rows, int NO, int n_in, int in_kind,
                                                               float *dW, int ld_dw, float *db) {
    __shared__ float part[16][64];
    const int per = NO * n_in + NO;
    const int t = threadIdx.x & 63, grp = threadIdx.x >> 6;      // 64 elements x 16 row groups
    const int e = blockIdx.x * 64 + t;
    float acc = 0.f;
    if (e < per) {
#pragma unroll 8
        for (int b = grp; b < n_rows; b += 16) acc += slab[(int64_t)b * per + e];
    }
    part[grp][t] = acc;
    __syncthreads();
    if (grp != 0 || e >= per) return;
#pragma unroll
    for (int k = 1; k < 16; ++k) acc += part[k][t];
    if (e < NO * n_in) {
        const int k = e / n_in, i = slot_to_feature(in_kind, e - k * n_in, 0);
        if (i >= 0) dW[(int64_t)k * ld_dw + i] = acc;
    } else {
        db[e - NO * n_in] = acc;
    }
}

// G [P, ldg] bf16 rows; columns g_col0 .. g_col0 + NO - 1 must lie inside one aligned group of four.
template <int NO>
static void launch_dw_small(hipStream_t s, int64_t P, float *slab, const uint16_t *G, int ldg, int g_col0, const uint16_t *X, int n_in,
                            float *dW, float *db) {
    int64_t g = (P + 255) / 256;
    if (g > 1024) g = 1024;    // four 256-thread blocks per CU keep enough 16-byte loads in flight; 1024 * (4 * 256 + 4) floats fit the slab
    hipLaunchKernelGGL(dw_small_kernel<NO>, dim3((unsigned)g), dim3(256), 0, s, G, ldg, g_col0, X, n_in, n_in, P, slab);
    hipLaunchKernelGGL(dw_small_reduce_kernel, dim3((NO * n_in + NO + 63) / 64), dim3(1024), 0, s, slab, (int)g, NO, n_in,
                       (int)PERM_ACC, dW, n_in, db);
}

// The cases of the two kernels' switch (J.shape) are the rows of DW_SHAPE (dw_plan.h); shape 5 is their default.
constexpr bool dw_switch_is_table = dw_shape_is(0, 16, 16, 4, 2, false) && dw_shape_is(1, 8, 16, 4, 2, false) && dw_shape_is(2, 16, 4, 8, 1, false) &&
                                    dw_shape_is(3, 8, 2, 8, 1, false) && dw_shape_is(4, 16, 16, 4, 2, true) && dw_shape_is(5, 0, 8, 0, 0, true) &&
                                    dw_shape_is(6, 16, 8, 4, 2, false) && dw_shape_is(7, 8, 4, 8, 1, false) && DW_SHAPES == 8;

// Every streaming product of one model's backward pass in ONE launch (dw_plan.h).  The job of a workgroup is the one whose
// range of blocks it lies in.  (Stamps build: the workgroup's start, its job and shape, and with HW_IDS the die and CU it
// runs on.)
template <bool HW_IDS>
__device__ __forceinline__ const DwJob &dw_job_of_block(const DwMulti &m) {
    int j = 0;
    while (j + 1 < m.n && (int)blockIdx.x >= m.job[j + 1].first_block) ++j;
    j = __builtin_amdgcn_readfirstlane(j);
    const DwJob &J = m.job[j];
#ifdef NERF_AMD_X_DW_STAMPS
    if (threadIdx.x == 0) {
        g_dw_stamps[4 * blockIdx.x] = wall_clock64();
        unsigned long long ids = 0;
        if (HW_IDS) {
            unsigned xcc, hwid;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
            ids = (unsigned long long)(xcc & 15) << 32 | (unsigned long long)(hwid & 0xffff) << 40;
        }
        g_dw_stamps[4 * blockIdx.x + 2] = (unsigned long long)j << 8 | (unsigned)J.shape | ids;
    }
#endif
    return J;
}

__global__ __launch_bounds__(512, 2) void dw_multi_kernel(DwMulti m) {
    const DwJob &J = dw_job_of_block<true>(m);
    const int wg = (int)blockIdx.x - J.first_block;
    static_assert(dw_switch_is_table, "the cases below are the rows of DW_SHAPE");
    switch (J.shape) {
    case 0: dw2_body<16, 16, 4, 2>(J.a, wg, J.n_blocks); break;
    case 1: dw2_body<8, 16, 4, 2>(J.a, wg, J.n_blocks); break;
    case 2: dw2_body<16, 4, 8, 1>(J.a, wg, J.n_blocks); break;
    case 3: dw2_body<8, 2, 8, 1>(J.a, wg, J.n_blocks); break;
    case 4: dw2_body<16, 16, 4, 2, true>(J.a, wg, J.n_blocks); break;
    case 6: dw2_body<16, 8, 4, 2>(J.a, wg, J.n_blocks); break;
    case 7: dw2_body<8, 4, 8, 1>(J.a, wg, J.n_blocks); break;
    default: dw_head_body<8>(J.a, wg, J.n_blocks); break;
    }
#ifdef NERF_AMD_X_DW_STAMPS
    __syncthreads();
    if (threadIdx.x == 0) g_dw_stamps[4 * blockIdx.x + 1] = wall_clock64();
#endif
}

// The same one launch for the split-precision products (dw2s_body, dw_head_split_body).
__global__ __launch_bounds__(512, 2) void dw_multi_split_kernel(DwMulti m) {
    const DwJob &J = dw_job_of_block<false>(m);
    const int wg = (int)blockIdx.x - J.first_block;
    static_assert(dw_switch_is_table, "the cases below are the rows of DW_SHAPE");
    switch (J.shape) {
    case 0: dw2s_body<16, 16, 4, 2>(J.a, wg, J.n_blocks); break;
    case 1: dw2s_body<8, 16, 4, 2>(J.a, wg, J.n_blocks); break;
    case 2: dw2s_body<16, 4, 8, 1>(J.a, wg, J.n_blocks); break;
    case 3: dw2s_body<8, 2, 8, 1>(J.a, wg, J.n_blocks); break;
    case 4: dw2s_body<16, 16, 4, 2, true>(J.a, wg, J.n_blocks); break;
    case 6: dw2s_body<16, 8, 4, 2>(J.a, wg, J.n_blocks); break;
    case 7: dw2s_body<8, 4, 8, 1>(J.a, wg, J.n_blocks); break;
    default: dw_head_split_body<8>(J.a, wg, J.n_blocks); break;
    }
#ifdef NERF_AMD_X_DW_STAMPS
    __syncthreads();
    if (threadIdx.x == 0) g_dw_stamps[4 * blockIdx.x + 1] = wall_clock64();
#endif
}

// output_linear's weight gradient in split precision (models without view branch, nerf.py:131-132): G = NO <= 4 columns
// of dL/draw itself (fp32, unscaled), X = the two planes of h8; fp32 FMA loops like dw_small_body.
template <int NO>
__global__ __launch_bounds__(256) void dw_small_split_kernel(const float *G, int ldg, int g_col0, const uint16_t *Xh, const uint16_t *Xl,
                                                             int ldx, int n_in, int64_t P, float *slab) {
    __shared__ float red[NO][256 + 1];
    const int groups = n_in / 8, rows_par = 256 / groups;
    const int cg = threadIdx.x % groups, ty = threadIdx.x / groups;
    const int wg = blockIdx.x, nwg = gridDim.x;
    float acc[NO][8], bs[NO];
#pragma unroll
    for (int k = 0; k < NO; ++k) {
        bs[k] = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[k][j] = 0.f;
    }
    for (int64_t r0 = (int64_t)wg * 256; r0 < P; r0 += (int64_t)nwg * 256) {
        const int64_t r1 = r0 + 256 < P ? r0 + 256 : P;
#pragma unroll 4
        for (int64_t p = r0 + ty; p < r1; p += rows_par) {
            const f16x8 xh = *reinterpret_cast<const f16x8 *>(Xh + p * ldx + cg * 8);
            const f16x8 xl = *reinterpret_cast<const f16x8 *>(Xl + p * ldx + cg * 8);
            float x[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = __builtin_fmaf((float)xl[j], SPLIT_INV, (float)xh[j]);
#pragma unroll
            for (int k = 0; k < NO; ++k) {
                const float g = G[p * ldg + g_col0 + k];
                if (cg == 0) bs[k] += g;
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[k][j] += g * x[j];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NO; ++k) red[k][threadIdx.x] = 0.f;
    if (threadIdx.x < NO) red[threadIdx.x][256] = 0.f;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NO; ++k) {
#pragma unroll
        for (int j = 0; j < 8; ++j) atomicAdd(&red[k][cg * 8 + j], acc[k][j]);
        if (cg == 0) atomicAdd(&red[k][256], bs[k]);
    }
    __syncthreads();
    float *row = slab + (int64_t)wg * (NO * n_in + NO);
    if ((int)threadIdx.x < n_in)
#pragma unroll
        for (int k = 0; k < NO; ++k) row[k * n_in + threadIdx.x] = red[k][threadIdx.x];
    if (threadIdx.x < NO) row[NO * n_in + threadIdx.x] = red[threadIdx.x][256];
}

// A job's slabs are few (~23), so one thread sums one element over all of them: DWR_BLOCK elements per block, no LDS, no
// barrier.
__global__ __launch_bounds__(DWR_BLOCK) void dw_reduce_multi_kernel(DwReduceMulti m) {
    int j = 0;
    while (j + 1 < m.n && (int)blockIdx.x >= m.first_block[j + 1]) ++j;
    j = __builtin_amdgcn_readfirstlane(j);
    const DwReduceArgs &a = m.r[j];
    const int per = dw_slab_floats(a.OT, a.IT, a.HT);
    const int e = ((int)blockIdx.x - m.first_block[j]) * DWR_BLOCK + (int)threadIdx.x;
    if (e >= per) return;
    float acc = 0.f;
#pragma unroll 8
    for (int b = 0; b < a.n_slabs; ++b) acc += a.slab[(int64_t)b * per + e];
    dw_scatter(a, e, acc);
}

namespace {
struct TrainWs {
    uint16_t *sv_e, *sv_d, *sv_h, *sv_feat, *sv_hv, *g_rawb, *g_rawt, *g_hv, *g_feat, *g_h;
    uint16_t *sv_e_lo, *sv_d_lo, *sv_h_lo, *sv_feat_lo, *sv_hv_lo, *g_rawt_lo, *g_hv_lo, *g_feat_lo, *g_h_lo;   // split: the lo planes
    uint8_t *sv_bits;
    float *g_scale;     // split: GRAD_SCALE_PARTS partial maxima of |dL/draw|, then S and 1 / S (split.h)
    float *slab;        // 2 x SLAB_FLOATS fp32: the slabs of the one launch's jobs, one after the other; the second half is
                        // the output_linear head's (a model without view branch), whose kernels may run beside the one launch
};
constexpr size_t SLAB_FLOATS = (size_t)256 * (256 * 256 + 256);
size_t al(size_t v) { return (v + 255) & ~(size_t)255; }

// Rows of a saved xyz-encoding row: 32 per k-step; a three-k-step encoding (multires 15) is padded to 128 so that its
// weight-gradient product keeps power-of-two rows and streams with the others in the one launch (dw2_body / dw2s_body; the
// extra slots are zero and map to no weight column).
int enc_row_slots(int k16) { return k16 == 3 ? 128 : 32 * k16; }

int64_t carve(const Program &p, int64_t P_points, char *base, TrainWs *w, bool split) {
    const size_t P = (size_t)pad_points(P_points);     // rows for the last workgroup's padding points too
    size_t off = 0;
    auto take = [&](size_t bytes) { char *q = base ? base + off : nullptr; off += al(bytes); return q; };
    auto lo = [&](size_t bytes) { return split ? (uint16_t *)take(bytes) : nullptr; };
    const size_t e = enc_row_slots(p.KE16), d = 32 * p.KD16;
    TrainWs t;
    t.sv_e = (uint16_t *)take(P * e * 2);              t.sv_e_lo = lo(P * e * 2);
    t.sv_d = (uint16_t *)take(P * d * 2);              t.sv_d_lo = lo(P * d * 2);
    t.sv_h = (uint16_t *)take((size_t)8 * P * 256 * 2); t.sv_h_lo = lo((size_t)8 * P * 256 * 2);
    t.sv_feat = (uint16_t *)take(P * 256 * 2);         t.sv_feat_lo = lo(P * 256 * 2);
    t.sv_hv = (uint16_t *)take(P * 128 * 2);           t.sv_hv_lo = lo(P * 128 * 2);
    t.sv_bits = (uint8_t *)take(P * (8 * 32 + 16));
    t.g_rawb = (uint16_t *)take(P * 16 * 2);           // [P, 4] with a view branch, [P, 16] without
    t.g_rawt = (uint16_t *)take(P * 4 * 2);            t.g_rawt_lo = lo(P * 4 * 2);
    t.g_hv = (uint16_t *)take(P * 128 * 2);            t.g_hv_lo = lo(P * 128 * 2);
    t.g_feat = (uint16_t *)take(P * 256 * 2);          t.g_feat_lo = lo(P * 256 * 2);
    t.g_h = (uint16_t *)take((size_t)8 * P * 256 * 2); t.g_h_lo = lo((size_t)8 * P * 256 * 2);
    t.g_scale = (float *)take((GRAD_SCALE_PARTS + 2) * sizeof(float));
    t.slab = (float *)take(2 * SLAB_FLOATS * sizeof(float));
    if (w) *w = t;
    return (int64_t)off;
}
}  // namespace

bool train_supported(const Program &p) {
    const nerf_amd_arch &a = p.arch;
    return fused_program(p) && family_known(a.multires, a.multires_views, a.use_viewdirs) && head_fits(a.use_viewdirs, p.out_ch);
}

int64_t train_workspace_bytes(const Program &p, int64_t P, bool split) { return carve(p, P, nullptr, nullptr, split); }

void train_fill_args(const Program &p, int64_t P, void *workspace, MlpArgs *a, bool split) {
    TrainWs w;
    carve(p, P, static_cast<char *>(workspace), &w, split);
    a->sv_e = w.sv_e; a->sv_d = w.sv_d; a->sv_h = w.sv_h; a->sv_feat = w.sv_feat; a->sv_hv = w.sv_hv;
    a->sv_bits = w.sv_bits;
    a->g_rawb = w.g_rawb; a->g_rawt = w.g_rawt; a->g_hv = w.g_hv; a->g_feat = w.g_feat; a->g_h = w.g_h;
    a->sv_e_lo = w.sv_e_lo; a->sv_d_lo = w.sv_d_lo; a->sv_h_lo = w.sv_h_lo; a->sv_feat_lo = w.sv_feat_lo; a->sv_hv_lo = w.sv_hv_lo;
    a->g_rawt_lo = w.g_rawt_lo; a->g_hv_lo = w.g_hv_lo; a->g_feat_lo = w.g_feat_lo; a->g_h_lo = w.g_h_lo;
    a->g_scale = w.g_scale;
}

// ... in split precision: G [P, ldg] fp32 rows, X as planes of fp16 hi and lo rows.
template <int NO>
static void launch_dw_small_split(hipStream_t s, int64_t P, float *slab, const float *G, int ldg, int g_col0, const uint16_t *Xh,
                                  const uint16_t *Xl, int n_in, float *dW, float *db) {
    int64_t g = (P + 255) / 256;
    if (g > 1024) g = 1024;
    hipLaunchKernelGGL(dw_small_split_kernel<NO>, dim3((unsigned)g), dim3(256), 0, s, G, ldg, g_col0, Xh, Xl, n_in, n_in, P, slab);
    hipLaunchKernelGGL(dw_small_reduce_kernel, dim3((NO * n_in + NO + 63) / 64), dim3(1024), 0, s, slab, (int)g, NO, n_in,
                       (int)PERM_ACC, dW, n_in, db);
}

// The products of one model as jobs of a plan, in launch order: layer 0, the layers after it (the one after the skip is two
// products, [input_pts | h]), and with a view branch feature_linear (alpha_linear riding along), views_linears.0 as
// [feature | dirs] and rgb_linear.  bf16 has no lo planes (carve leaves them NULL) and no loss scale to take off.
static int plan_weight_grads(DwPlan &plan, const Program &p, int64_t P, const TrainWs &w, float *const *gw, float *const *gb, bool split) {
    const int D = p.arch.D, W = p.arch.W, E = enc_row_slots(p.KE16), Dd = 32 * p.KD16, ic = p.input_ch, icv = p.input_ch_views;
    const bool vd = p.arch.use_viewdirs != 0;
    if (W != 256 || (E != 64 && E != 128) || (vd && Dd != 32 && Dd != 64)) return NERF_AMD_EUNSUPPORTED;
    const int Lx = p.arch.multires, Ld = p.arch.multires_views;
    const int64_t HS = pad_points(P) * 256;
    const float *inv_scale = split ? w.g_scale + GRAD_SCALE_PARTS + 1 : nullptr;
    auto rows = [](const uint16_t *hi, const uint16_t *lo, int64_t off = 0) { return DwPlanes{hi + off, lo ? lo + off : nullptr}; };
    int rc = NERF_AMD_OK;
    // dW[:, col_off : col_off + m_valid] (+ db) of one Linear from G [P, n_out_slots] and X [P, n_in_slots]
    auto product = [&](DwPlanes X, int n_in_slots, int in_kind, int in_L, int m_valid, DwPlanes G, int n_out_slots, float *dW, int ld_dw,
                       int col_off, float *db, const DwHead *head = nullptr) {
        if (!rc) rc = plan.add(P, X, n_in_slots, in_kind, in_L, m_valid, G, n_out_slots, n_out_slots, dW, ld_dw, col_off, db, head, inv_scale);
    };
    const DwPlanes Xe = rows(w.sv_e, w.sv_e_lo);
    for (int l = 0; l < D; ++l) {
        const DwPlanes G = rows(w.g_h, w.g_h_lo, l * HS), Xh = rows(w.sv_h, w.sv_h_lo, (l > 0 ? l - 1 : 0) * HS);
        const int n_in = p.tensors[l].n_in;
        if (l == 0) {
            product(Xe, E, PERM_GEN, Lx, ic, G, W, gw[l], n_in, 0, gb[l]);
        } else if (n_in == W + ic) {      // the layer after the skip: [input_pts | h]
            product(Xe, E, PERM_GEN, Lx, ic, G, W, gw[l], n_in, 0, nullptr);
            product(Xh, W, PERM_ACC, 0, W, G, W, gw[l], n_in, ic, gb[l]);
        } else {
            product(Xh, W, PERM_ACC, 0, W, G, W, gw[l], n_in, 0, gb[l]);
        }
    }
    if (vd) {
        const DwPlanes Ghv = rows(w.g_hv, w.g_hv_lo), H = rows(w.g_rawt, w.g_rawt_lo);
        // feature_linear -- and alpha_linear, whose product has the same X (h8): its gradient column rides along as a head
        // tile (row 3 of dL/draw's columns) instead of a separate kernel re-reading h8
        const DwHead alpha_head{H, 3, 1, W, gw[D + 1], gb[D + 1]};
        product(rows(w.sv_h, w.sv_h_lo, (D - 1) * HS), W, PERM_ACC, 0, W, rows(w.g_feat, w.g_feat_lo), W, gw[D], W, 0, gb[D], &alpha_head);
        // views_linears.0: [feature | dirs]
        product(rows(w.sv_feat, w.sv_feat_lo), W, PERM_ACC, 0, W, Ghv, W / 2, gw[D + 2], W + icv, 0, gb[D + 2]);
        product(rows(w.sv_d, w.sv_d_lo), Dd, PERM_GEN, Ld, icv, Ghv, W / 2, gw[D + 2], W + icv, W, nullptr);
        // rgb_linear: rows 0..2 of dL/draw's columns over the view layer's output; nothing else multiplies that output, so
        // the head is a job of its own
        const DwHead rgb_head{H, 0, 3, W / 2, gw[D + 3], gb[D + 3]};
        product(rows(w.sv_hv, w.sv_hv_lo), W / 2, PERM_ACC, 0, W / 2, DwPlanes{nullptr, nullptr}, 0, nullptr, 0, 0, nullptr, &rgb_head);
    }
    return rc;
}

// A laid-out plan: one launch of K for the jobs with lds bytes of dynamic LDS, one for their reductions.
template <void (*K)(DwMulti)>
static int launch_plan(const DwPlan &plan, size_t lds, hipStream_t stream) {
    if (lds > DW_LDS_MAX) return NERF_AMD_EINVAL;
    static DynamicLdsOptIn opt_in;
    if (opt_in.ensure(reinterpret_cast<const void *>(K), DW_LDS_MAX) != hipSuccess) return NERF_AMD_EHIP;
    hipLaunchKernelGGL(K, dim3((unsigned)plan.n_blocks()), dim3(512), lds, stream, plan.mj);
    hipLaunchKernelGGL(dw_reduce_multi_kernel, dim3((unsigned)plan.n_reduce_blocks()), dim3(DWR_BLOCK), 0, stream, plan.mr);
    return NERF_AMD_OK;
}

// output_linear [out_ch, W] of a model without view branch (nerf.py:131-132): X = h8, four rows per launch.  G = the
// out_ch <= 16 columns of g_rawb [P, 16], or in split precision of dL/draw itself (fp32, unscaled).  The slabs are the
// second half of the slab buffer (1024 x (4 x 256 + 4) floats), so the kernels may run beside the one launch.
static void output_head_grads(const Program &p, int64_t P, const TrainWs &w, float *const *gw, float *const *gb, const float *g_raw, bool split,
                              hipStream_t s) {
    const int D = p.arch.D, W = p.arch.W;
    const int64_t HS = pad_points(P) * 256;
    const uint16_t *h8 = w.sv_h + (D - 1) * HS, *h8_lo = split ? w.sv_h_lo + (D - 1) * HS : nullptr;
    float *slab = w.slab + SLAB_FLOATS;
    for (int r0 = 0; r0 < p.out_ch; r0 += 4) {
        float *dWr = gw[D] + (int64_t)r0 * W, *dbr = gb[D] + r0;
        auto launch = [&](auto no) {
            constexpr int NO = decltype(no)::value;
            if (split) launch_dw_small_split<NO>(s, P, slab, g_raw, p.out_ch, r0, h8, h8_lo, W, dWr, dbr);
            else launch_dw_small<NO>(s, P, slab, w.g_rawb, 16, r0, h8, W, dWr, dbr);
        };
        switch (p.out_ch - r0) {
        case 1: launch(std::integral_constant<int, 1>{}); break;
        case 2: launch(std::integral_constant<int, 2>{}); break;
        case 3: launch(std::integral_constant<int, 3>{}); break;
        default: launch(std::integral_constant<int, 4>{}); break;
        }
    }
}

// Parameter gradients of the model from the saved activations and the pre-activation gradients the dX-chain kernel left in
// the workspace.  Every product overwrites its destination (no accumulation into gw / gb).
int train_param_grads(const Program &p, int64_t P, void *workspace, float *const *gw, float *const *gb, int device, hipStream_t stream,
                      bool split, const float *g_raw) {
    TrainWs w;
    carve(p, P, static_cast<char *>(workspace), &w, split);
    DwPlan plan;
    if (const int rc = plan_weight_grads(plan, p, P, w, gw, gb, split)) return rc;
    plan.layout(P, w.slab, split);
    const bool head = p.arch.use_viewdirs == 0;        // output_linear: not a job of the plan
    if (split) {
        // the reduction also takes the loss scale off; the head follows it on the caller's stream
        if (const int rc = launch_plan<dw_multi_split_kernel>(plan, plan.lds, stream)) return rc;
        if (head) output_head_grads(p, P, w, gw, gb, g_raw, true, stream);
        return hipGetLastError() == hipSuccess ? NERF_AMD_OK : NERF_AMD_EHIP;
    }
    // bf16: the head runs on the library's side stream beside the one launch (fp32 FMA kernels whose small blocks share a CU
    // with a streaming workgroup), forked before it and joined after it; without events, behind it on the caller's stream
    hipStream_t side = nullptr;
    std::vector<hipEvent_t> ev;
    const bool beside = head && lane_acquire(device, 2, &side, &ev) == NERF_AMD_OK;
    if (beside) {
        (void)hipEventRecord(ev[0], stream);
        (void)hipStreamWaitEvent(side, ev[0], 0);
        output_head_grads(p, P, w, gw, gb, g_raw, false, side);
    }
    const int rc = launch_plan<dw_multi_kernel>(plan, DW_LDS_MAX, stream);
    if (beside) {
        (void)hipEventRecord(ev[1], side);
        (void)hipStreamWaitEvent(stream, ev[1], 0);
        lane_release(device, ev);
    }
    if (rc) return rc;
    if (head && !beside) output_head_grads(p, P, w, gw, gb, g_raw, false, stream);
    return hipGetLastError() == hipSuccess ? NERF_AMD_OK : NERF_AMD_EHIP;
}

}  // namespace na
