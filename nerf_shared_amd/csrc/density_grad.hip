// density_grad.hip -- sigma and d(sigma)/d(point) of a frozen field in ONE launch, without a workspace
// (NeRF.density_and_grad; nerf_amd_density_value_grad), for the models without a view branch of the fused family
// (D=8, W=256, skips=[4]; a density twin, or an output_linear model whose last channel is sigma), in bf16.
//
// The kernel is the two kernels a training step runs, back to back on one 256-point tile:
//   forward   mlp_bf16_s16_kernel<LX, 0, false>: encodings in registers, eight hidden layers, the head -- same fragments,
//             same order, same rounding; sigma = row out_ch - 1 of the head tile;
//   backward  mlp_bwd_s16_kernel<LX, 0, false, C, RAYG = true>'s chain with dL/draw = 1 in the sigma column: the
//             transposed products, ReLU masks, the two encoding products, encode16_bwd, one lane per point writes.
// What a training step sends through HBM between the two stays on chip: the "activation > 0" bits (8 layers x 256 bits
// per point) go to LDS -- 8 KiB per wave beside the 64-KiB ring, every wave reads back only what it wrote, so no barrier
// guards them -- and no g_pre(l) row is stored, because no weight-gradient product follows.
// Ring: the two weight streams pass through the same ring one after the other.  The forward ends like every tile of the
// simple forward kernel (vmcnt(0), workgroup barrier: nothing in flight, every wave done reading), then the backward
// stream starts with its own prologue.  Neither half issues global stores between its syncs, so the counted waits of
// pipeline.h hold with the empty ledger.
#include <hip/hip_runtime.h>
#include <utility>

#include "kernels.h"
#include "launch_util.h"
#include "pipeline.h"
#include "program.h"

// the device templates of the two kernels this one is made of (tile_pair, layer16, encode16 / tpair, pack_grad, tenc,
// encode16_bwd and the fragment layouts), without their launchers
#define NA_DEVICE_TEMPLATES_ONLY
#include "mlp_bf16_s16.hip"
#include "mlp_bwd_s16.hip"

namespace na {

// The mask words save_bits (mlp_bf16_s16.hip) would store for column tile CC of a 256-wide layer: the same bit layout,
// so pack_grad reads them as it reads the saved rows.
template <int CC>
__device__ __forceinline__ void mask_words(const bf16x8 *y, unsigned (&w)[2]) {
    w[0] = 0; w[1] = 0;
    static_for<8>([&](auto k_) {
        constexpr int k = k_;
        const u32x4 v = __builtin_bit_cast(u32x4, y[2 * k + CC]);
        unsigned t = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            unsigned m;
            asm("v_pk_min_u16 %0, %1, %2" : "=v"(m) : "v"(v[i]), "v"(0x00010001u));   // 1 per non-zero half
            t |= m << i;
        }
        w[k / 4] |= t << (4 * (k % 4));
    });
}

// This lane's mask words of layer L in the wave's LDS block: [layer][column tile][dword][lane], conflict-free.
template <int L>
__device__ __forceinline__ void keep_bits(unsigned *wave_bits, const bf16x8 *y, int lane) {
    static_for<2>([&](auto cc_) {
        constexpr int cc = cc_;
        unsigned w[2];
        mask_words<cc>(y, w);
        wave_bits[((L * 2 + cc) * 2 + 0) * 64 + lane] = w[0];
        wave_bits[((L * 2 + cc) * 2 + 1) * 64 + lane] = w[1];
    });
}
template <int L>
__device__ __forceinline__ MaskBits<8> kept_bits(const unsigned *wave_bits, int lane) {
    MaskBits<8> m;
    static_for<2>([&](auto cc_) {
        constexpr int cc = cc_;
        m.w[cc][0] = wave_bits[((L * 2 + cc) * 2 + 0) * 64 + lane];
        m.w[cc][1] = wave_bits[((L * 2 + cc) * 2 + 1) * 64 + lane];
    });
    return m;
}

// tlayer of mlp_bwd_s16.hip without its row stores: the masked bf16 gradient fragments stay in registers.
template <int F0, int K1, int NB, int NFRAGS, class C>
__device__ __forceinline__ void tlayer_reg(C &c, const bf16x8 *x, bf16x8 *g, const MaskBits<8> &mask) {
    static_for<8>([&](auto p_) {
        constexpr int p = p_;
        f32x4 acc[2][2];
        tpair<F0 + p * 2 * K1, K1, 0, NB, NFRAGS>(c, x, x, acc);
        g[2 * p] = pack_grad<true, 4 * (p % 4)>(acc[0][0], acc[1][0], mask.w[0][p / 4]);
        g[2 * p + 1] = pack_grad<true, 4 * (p % 4)>(acc[0][1], acc[1][1], mask.w[1][p / 4]);
    });
}

constexpr int DG_BITS_BYTES_PER_WAVE = 8 * 2 * 2 * 64 * 4;      // 8 KiB

template <int LX, class C>
__global__ __launch_bounds__(C::WAVES * 64, 2) void mlp_density_grad_kernel(MlpArgs a) {
    constexpr int WG_THREADS = C::WAVES * 64, WG_POINTS = C::WAVES * 32;
    using Lay = Layout16<LX, 0, false>;
    constexpr int KE = Lay::KE, NF = Lay::F_END, NB = (NF + C::BF - 1) / C::BF;
    using LB = LayoutB<KE, 1, false>;
    constexpr int NFB = LB::F_END, NBB = (NFB + C::BF - 1) / C::BF;
    static_assert(C::PHASE > 0 && std::is_same<typename C::Ledger, NoLedger>::value, "no stores are counted into the ring's waits");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *bias_lds = reinterpret_cast<float *>(smem + C::RING_BYTES);
    constexpr int BIAS_BYTES = Lay::N_TILES * 16 * (int)sizeof(float);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int q = lane >> 4;
    C c;
    c.wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    c.lag = 0;
    c.phase = 0;
    c.gstream = reinterpret_cast<const char *>(a.stream_s16) + lane * 16;
    c.ring_lane = smem + lane * 16;
    c.ring_u32 = (uint32_t)(uintptr_t)smem;
    c.bias_half = bias_lds + q * 4;          // this lane's 4 rows of every 16-row tile
    unsigned *wave_bits = reinterpret_cast<unsigned *>(smem + C::RING_BYTES + BIAS_BYTES + c.wave * DG_BITS_BYTES_PER_WAVE);

    for (int i = tid; i < Lay::N_TILES * 16; i += WG_THREADS) bias_lds[i] = a.bias_s16[i];

    // ================================================================ forward (mlp_bf16_s16_kernel, VD = false)
    pipeline_prologue<NB>(c);
    bf16x8 E[KE * 2];
    int64_t pidx[2];
    bool valid[2];
    float xs[2][3];
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
        const int64_t p = (int64_t)blockIdx.x * WG_POINTS + c.wave * 32 + cc * 16 + (lane & 15);
        pidx[cc] = p;
        valid[cc] = p < a.P;
        const int64_t pc = valid[cc] ? p : a.P - 1;
        xs[cc][0] = a.pts[3 * pc + 0]; xs[cc][1] = a.pts[3 * pc + 1]; xs[cc][2] = a.pts[3 * pc + 2];
    }
    static_for<2>([&](auto cc_) {
        constexpr int cc = cc_;
        encode16<LX, KE, 2>(xs[cc][0], xs[cc][1], xs[cc][2], q >> 1, q & 1, E + cc);
    });
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // bias table stores, before the barrier publishes them
    block_sync<-1, NB>(c);                                 // publishes block 0
    static_for<C::LA>([&](auto i_) { constexpr int i = i_; c.q[i] = ring_frag<i>(c); });

    bf16x8 A[16], B[16];
    layer16<Lay::F_L0, 0, 8, KE, 0, true, NB, NF>(c, E, E, A);
    keep_bits<0>(wave_bits, A, lane);
    layer16<Lay::F_L1 + 0 * 128, 16, 8, 8, 0, true, NB, NF>(c, A, A, B);
    keep_bits<1>(wave_bits, B, lane);
    layer16<Lay::F_L1 + 1 * 128, 32, 8, 8, 0, true, NB, NF>(c, B, B, A);
    keep_bits<2>(wave_bits, A, lane);
    layer16<Lay::F_L1 + 2 * 128, 48, 8, 8, 0, true, NB, NF>(c, A, A, B);
    keep_bits<3>(wave_bits, B, lane);
    layer16<Lay::F_L1 + 3 * 128, 64, 8, 8, 0, true, NB, NF>(c, B, B, A);
    keep_bits<4>(wave_bits, A, lane);
    layer16<Lay::F_L5, 80, 8, KE, 8, true, NB, NF>(c, E, A, B);            // skip: [input_pts | h]
    keep_bits<5>(wave_bits, B, lane);
    layer16<Lay::F_L6, 96, 8, 8, 0, true, NB, NF>(c, B, B, A);
    keep_bits<6>(wave_bits, A, lane);
    layer16<Lay::F_L6 + 128, 112, 8, 8, 0, true, NB, NF>(c, A, A, B);      // h7 in B
    keep_bits<7>(wave_bits, B, lane);
    {
        f32x4 o[2];
        tile_single<Lay::F_HEAD, 128, 8, NB, NF>(c, B, o);
        static_for<2>([&](auto cc_) {
            constexpr int cc = cc_;
            if (valid[cc]) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (4 * q + r == a.out_ch - 1) a.out[pidx[cc]] = o[cc][r];     // sigma: the last channel
            }
        });
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // no LDS-DMA of the forward stream is in flight ...
    __syncthreads();                                           // ... and every wave is done reading the ring

    // ================================================================ backward (mlp_bwd_s16_kernel's chain, VD = false, RAYG)
    c.gstream = reinterpret_cast<const char *>(a.stream_bwd) + lane * 16;
    c.bias_half = nullptr;
    pipeline_prologue<NBB>(c);
    // dL/draw as the FRAG_TG16 operand: k slot (q, j) = output_linear row 8 q + j; 1 in the sigma row of a real point
    bf16x8 Gsig[2];
    static_for<2>([&](auto cc_) {
        constexpr int cc = cc_;
        bf16x8 o = {};
        if (q < 2) {
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (__bf16)((valid[cc] && 8 * q + j == a.out_ch - 1) ? 1.0f : 0.0f);
        }
        Gsig[cc] = o;
    });
    block_sync<-1, NBB>(c);
    static_for<C::LA>([&](auto i_) { constexpr int i = i_; c.q[i] = ring_frag<i>(c); });

    const int hh = q >> 1, bb = q & 1;
    float gx[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
    // the mask words are read one layer ahead of their use, as the chain kernel loads its bit rows
    MaskBits<8> m_cur = kept_bits<7>(wave_bits, lane), m_next = kept_bits<6>(wave_bits, lane);
    // g_h8 = relu'(h8) * (W_output^T dL/draw)
    tlayer_reg<LB::F_H8, 1, NBB, NFB>(c, Gsig, B, m_cur);
    // g_h(l-1) = relu'(h(l-1)) * (W_l^T g_h(l)),  l = 7 .. 1   (layer 5 uses the h-columns of its [e | h] input)
    m_cur = m_next; m_next = kept_bits<5>(wave_bits, lane);
    tlayer_reg<LB::F_L7 + 0 * 128, 8, NBB, NFB>(c, B, A, m_cur);
    m_cur = m_next; m_next = kept_bits<4>(wave_bits, lane);
    tlayer_reg<LB::F_L7 + 1 * 128, 8, NBB, NFB>(c, A, B, m_cur);
    m_cur = m_next; m_next = kept_bits<3>(wave_bits, lane);
    tlayer_reg<LB::F_L7 + 2 * 128, 8, NBB, NFB>(c, B, A, m_cur);
    {   // xyz encoding through the skip layer's [input_pts] columns (its pre-activation gradient is still in B)
        float g[2][8 * KE];
        tenc<LB::F_E5, KE, 8, NBB, NFB>(c, B, g);
        static_for<2>([&](auto cc_) { constexpr int cc = cc_; encode16_bwd<LX, KE>(xs[cc][0], xs[cc][1], xs[cc][2], hh, bb, g[cc], gx[cc]); });
    }
    m_cur = m_next; m_next = kept_bits<2>(wave_bits, lane);
    tlayer_reg<LB::F_L4 + 0 * 128, 8, NBB, NFB>(c, A, B, m_cur);
    m_cur = m_next; m_next = kept_bits<1>(wave_bits, lane);
    tlayer_reg<LB::F_L4 + 1 * 128, 8, NBB, NFB>(c, B, A, m_cur);
    m_cur = m_next; m_next = kept_bits<0>(wave_bits, lane);
    tlayer_reg<LB::F_L4 + 2 * 128, 8, NBB, NFB>(c, A, B, m_cur);
    m_cur = m_next;
    tlayer_reg<LB::F_L4 + 3 * 128, 8, NBB, NFB>(c, B, A, m_cur);
    {   // xyz encoding through pts_linears.0
        float g[2][8 * KE];
        tenc<LB::F_E0, KE, 8, NBB, NFB>(c, A, g);
        static_for<2>([&](auto cc_) { constexpr int cc = cc_; encode16_bwd<LX, KE>(xs[cc][0], xs[cc][1], xs[cc][2], hh, bb, g[cc], gx[cc]); });
    }
    // ---- sum the four lane quarters of each point, then one lane per point writes (no atomics)
    static_for<2>([&](auto cc_) {
        constexpr int cc = cc_;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            gx[cc][k] += __shfl_xor(gx[cc][k], 16); gx[cc][k] += __shfl_xor(gx[cc][k], 32);
        }
        if (valid[cc] && q == 0) {
            a.g_pts[3 * pidx[cc]] = gx[cc][0]; a.g_pts[3 * pidx[cc] + 1] = gx[cc][1]; a.g_pts[3 * pidx[cc] + 2] = gx[cc][2];
        }
    });
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // no LDS-DMA may outlive the workgroup
}

// The pipeline shape of the training forward and of the chain kernel (round-1 shape), empty ledger.
using CfgDG = Ctx<8, 16, 4, 8, 2>;

template <int LX>
static int launch_dg(const MlpArgs &a, int n_frags_fwd, int n_tiles, int n_frags_bwd, hipStream_t s) {
    using Lay = Layout16<LX, 0, false>;
    using LB = LayoutB<gen16_ksteps(LX), 1, false>;
    if (n_frags_fwd != Lay::F_END || n_tiles != Lay::N_TILES || n_frags_bwd != LB::F_END) return NERF_AMD_EINVAL;
    if (a.P <= 0) return NERF_AMD_OK;
    if (a.P >= (int64_t)1 << 31 || a.out_ch < 1 || a.out_ch > 16 || !a.pts || !a.out || !a.g_pts) return NERF_AMD_EINVAL;
    const size_t lds = CfgDG::RING_BYTES + (size_t)Lay::N_TILES * 16 * sizeof(float) + (size_t)CfgDG::WAVES * DG_BITS_BYTES_PER_WAVE;
    static_assert(CfgDG::RING_BYTES + Lay::N_TILES * 16 * sizeof(float) + CfgDG::WAVES * DG_BITS_BYTES_PER_WAVE <= LDS_LIMIT_BYTES, "one workgroup per CU");
    static DynamicLdsOptIn opt_in;
    // one 256-point tile per workgroup, like the chain kernel: no tile loop, no tickets
    return launch_field({reinterpret_cast<const void *>(mlp_density_grad_kernel<LX, CfgDG>), &opt_in, lds, 512, 256, 0}, a, s);
}

// Shipped: multires 10 (250 VGPRs, no scratch).  The multires-15 instantiation needs the 24-slot encoding products beside
// the chain's 128 fragment registers and spills 111 VGPRs at the 256 a wave of an 8-wave workgroup can have (DESIGN.md
// section 8d), like the RAYG chain kernel it is made of: such models take the two-launch route.
constexpr int DG_MULTIRES = 10;
bool density_grad_fused_supported(int multires, int use_viewdirs, int out_ch) {
    return !use_viewdirs && family_known(multires, 0, 0) && multires == DG_MULTIRES && out_ch >= 1 && head_fits(false, out_ch);
}

int launch_density_grad(const MlpArgs &a, int multires, int n_frags_fwd, int n_tiles, int n_frags_bwd, hipStream_t s) {
    return for_family(multires, 0, 0, [&](auto f) -> int {
        if constexpr (f.lx == DG_MULTIRES) return launch_dg<f.lx>(a, n_frags_fwd, n_tiles, n_frags_bwd, s);
        return NERF_AMD_EUNSUPPORTED;
    });
}

// ---- the two element-wise helpers of the density entry points for output_linear models with more than one channel
__global__ void density_last_channel_kernel(const float *raw, int64_t n, int out_ch, float *sigma) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sigma[i] = raw[i * out_ch + (out_ch - 1)];
}
// dL/draw of sum(sigma): 1 in the last channel of every point, 0 elsewhere
__global__ void density_unit_grad_kernel(float *g_raw, int64_t n, int out_ch) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n * out_ch) g_raw[i] = (i % out_ch == out_ch - 1) ? 1.0f : 0.0f;
}

int launch_density_last_channel(const float *raw, int64_t n, int out_ch, float *sigma, hipStream_t s) {
    if (n <= 0) return NERF_AMD_OK;
    hipLaunchKernelGGL(density_last_channel_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, raw, n, out_ch, sigma);
    return hipGetLastError() == hipSuccess ? NERF_AMD_OK : NERF_AMD_EHIP;
}
int launch_density_unit_grad(float *g_raw, int64_t n, int out_ch, hipStream_t s) {
    if (n <= 0) return NERF_AMD_OK;
    hipLaunchKernelGGL(density_unit_grad_kernel, dim3((unsigned)((n * out_ch + 255) / 256)), dim3(256), 0, s, g_raw, n, out_ch);
    return hipGetLastError() == hipSuccess ? NERF_AMD_OK : NERF_AMD_EHIP;
}

}  // namespace na
