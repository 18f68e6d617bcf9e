// pack.hip -- re-pack live nn.Linear parameters ([out,in] fp32, state_dict
// layout of /root/reference/nerf_shared/nerf.py:62-94) into the fragment
// streams of program.h, on the device (no host sync), plus the host twin used
// by the CPU layout tests.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "program.h"

namespace na {

NA_HD inline uint16_t f32_to_bf16_rne(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// fp32 -> IEEE fp16 bits, round to nearest even (overflow -> inf), by hand: shared by the host twin, whose toolchain
// may lack the _Float16 conversion routines.
NA_HD inline uint16_t f32_to_f16_rne(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    const uint32_t sign = (u >> 16) & 0x8000u;
    u &= 0x7fffffffu;
    if (u > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);                 // NaN
    if (u >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                // rounds to >= 65520: inf
    if (u < 0x38800000u) {                                                  // |f| < 2^-14: fp16 denormal or zero
        if (u < 0x33000000u) return (uint16_t)sign;                         // < 2^-25: zero
        const int e = (int)(u >> 23);                                       // biased fp32 exponent, 102..112
        uint32_t m = (u & 0x7fffffu) | 0x800000u;                           // 24-bit significand
        const int shift = 126 - e;                                          // 14..24: significand >> shift = multiples of 2^-24
        const uint32_t half = 1u << (shift - 1), rest = m & ((1u << shift) - 1u);
        m >>= shift;
        if (rest > half || (rest == half && (m & 1u))) ++m;
        return (uint16_t)(sign | m);
    }
    u += 0xc8000000u;                                                       // re-bias the exponent: -(127 - 15) << 23
    u += 0x0fffu + ((u >> 13) & 1u);
    return (uint16_t)(sign | (u >> 13));
}
NA_HD inline float f16_bits_to_f32(uint16_t h) {
    const uint32_t sign = ((uint32_t)h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
    uint32_t u;
    if (e == 0) {
        if (m == 0) u = sign;
        else {                                                              // denormal: normalise
            int k = 0;
            uint32_t mm = m;
            while (!(mm & 0x400u)) { mm <<= 1; ++k; }
            u = sign | ((uint32_t)(113 - k) << 23) | ((mm & 0x3ffu) << 13);
        }
    } else if (e == 31) u = sign | 0x7f800000u | (m << 13);
    else u = sign | ((e + 112u) << 23) | (m << 13);
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
// Element of a fragment of `part` (program.h FragDesc): bf16(w), or the fp16 pair of the split-precision stream --
// hi = fp16(w) (0 where that would be a denormal, so no operand ever is one), lo = fp16((w - hi) 2^11).
NA_HD inline uint16_t pack_value(float w, int part) {
    if (part == 0) return f32_to_bf16_rne(w);
    uint16_t hi = f32_to_f16_rne(w);
    if ((hi & 0x7c00u) == 0) hi = 0;
    if (part == 1) return hi;
    return f32_to_f16_rne((w - f16_bits_to_f32(hi)) * 2048.0f);
}

// Weight column (inside the tensor) held by element j of lane `lane` of fragment d, or -1.
NA_HD inline int frag_source(const FragDesc &d, int lane, int j, int n_out, int *row) {
    if (d.kind == FRAG_T16 || d.kind == FRAG_TG16 || d.kind == FRAG_TE16) {   // transposed: *row = output feature, column = input feature
        const int i = lane & 15, q = lane >> 4;
        const int o = d.kind == FRAG_TG16 ? 32 * d.ks + 8 * q + j : acc16_col(d.ks, q, j);
        *row = o;
        if (o >= d.seg_len) return -1;
        if (d.kind == FRAG_TE16) {       // tile row i = encoding slot (ks' = t>>1, q' = i>>2, j' = 4(t&1) + (i&3))
            const int t = d.row0 >> 4;
            const int c = gen16_col(t >> 1, i >> 2, 4 * (t & 1) + (i & 3), d.L);
            return c < 0 ? -1 : d.col_base + c;
        }
        if (d.row0 + i >= d.L) return -1;
        return d.col_base + d.row0 + i;
    }
    const bool s16 = d.kind == FRAG_ACC16 || d.kind == FRAG_GEN16;
    const int o = s16 ? (lane & 15) : (lane & 31), h = s16 ? (lane >> 4) : (lane >> 5);
    *row = d.row0 + o;
    if (d.kind == FRAG_ZERO || *row >= n_out) return -1;
    const int c = d.kind == FRAG_GEN ? gen_col(d.ks, h, j, d.L)
                : d.kind == FRAG_ACC ? acc_col(d.ks, h, j)
                : d.kind == FRAG_GEN16 ? gen16_col(d.ks, h, j, d.L) : acc16_col(d.ks, h, j);
    if (c < 0 || c >= d.seg_len) return -1;
    return d.col_base + c;
}

// Element (lane, j) of fragment d, packed from the tensor it names.
NA_HD inline uint16_t frag_value(const FragDesc d, int lane, int j, const TensorDesc *tensors, const float *const *weights) {
    int row;
    const TensorDesc t = tensors[d.tensor];
    const int col = frag_source(d, lane, j, t.n_out, &row);
    return pack_value(col < 0 ? 0.0f : weights[d.tensor][(int64_t)row * t.n_in + col], d.part);
}
// Element e of a bias table of `rows`-row tiles (program.h STREAMS: 16 natural rows, or the 32 of a 32x32x16 tile as [h][r]).
NA_HD inline float bias_value(const TileDesc *tiles, int rows, int e, const TensorDesc *tensors, const float *const *biases) {
    const TileDesc t = tiles[e >> (rows == 32 ? 5 : 4)];
    const int row = t.row0 + bias_tile_row(e & (rows - 1), rows);
    return row < tensors[t.tensor].n_out ? biases[t.tensor][row] : 0.0f;
}

// Every packed copy of a model from ONE launch (a re-pack follows every optimizer step of a training loop, where six
// small launches cost more on the host than on the GPU).  Per stream of program.h a fragment job (one block per fragment)
// and a bias job (512 elements per block); the launcher lays their block ranges out one after the other and hands the
// kernel the end of each (a job that is not asked for ends where it starts), side by side in front of the arguments: a
// block finds its job with one load.
struct FragJob { const FragDesc *frags; uint16_t *out; };
struct BiasJob { const TileDesc *tiles; float *out; int n, rows; };              // n elements in tiles of `rows` rows
struct PackJobs {
    int end[2 * N_STREAMS];          // first block behind fragment job i, then behind bias job i
    const TensorDesc *tensors;
    FragJob frag[N_STREAMS];
    BiasJob bias[N_STREAMS];
    const LayerF32 *layers;          // the fp32 streams: from block end[2 * N_STREAMS - 1] on
    const TrainLayerF32 *tlayers;
    float *stream_f32, *bias_f32, *stream_f32_t;
    int n_layers, n_layers_t;
};
constexpr int PACK_F32_BLOCKS = 32;  // per layer
static_assert(sizeof(PackJobs) + 2 * sizeof(PtrTable) <= 4096, "kernel-argument block of pack_all_kernel");

__global__ __launch_bounds__(512) void pack_all_kernel(PackJobs J, PtrTable weights_tab, PtrTable biases_tab) {
    const float *const *weights = weights_tab.p;
    const float *const *biases = biases_tab.p;
    int b = blockIdx.x;
    // Unrolled: every job is read from the kernel arguments at a compile-time offset, so J is never copied to scratch.  One
    // test finds the kind of job, then one copy of the packing code runs on the job picked among its kind.
    if (b < J.end[N_STREAMS - 1]) {
        FragJob fj = J.frag[0];
#pragma unroll
        for (int i = 1; i < N_STREAMS; ++i)
            if ((int)blockIdx.x >= J.end[i - 1]) { fj = J.frag[i]; b = blockIdx.x - J.end[i - 1]; }
        fj.out[(int64_t)b * 512 + threadIdx.x] = frag_value(fj.frags[b], threadIdx.x >> 3, threadIdx.x & 7, J.tensors, weights);
        return;
    }
    if (b < J.end[2 * N_STREAMS - 1]) {
        BiasJob bj = J.bias[0];
        b -= J.end[N_STREAMS - 1];
#pragma unroll
        for (int i = 1; i < N_STREAMS; ++i)
            if ((int)blockIdx.x >= J.end[N_STREAMS + i - 1]) { bj = J.bias[i]; b = blockIdx.x - J.end[N_STREAMS + i - 1]; }
        const int e = b * 512 + threadIdx.x;
        if (e < bj.n) bj.out[e] = bias_value(bj.tiles, bj.rows, e, J.tensors, biases);
        return;
    }
    b -= J.end[2 * N_STREAMS - 1];
    // fp32 stream: blocks of 256 values = one (tile, group) of a layer; a 512-thread block packs two at a time
    if (b >= J.n_layers * PACK_F32_BLOCKS) {
        // the transposed fp32 stream of train_f32.hip: tiles over the layer's INPUT features, k over its outputs
        b -= J.n_layers * PACK_F32_BLOCKS;
        const int layer = b / PACK_F32_BLOCKS, bx = b - layer * PACK_F32_BLOCKS;
        if (layer >= J.n_layers_t) return;
        const LayerF32 L = J.layers[layer];
        const int tiles = (L.n_in + 31) >> 5, groups = (L.n_out + 7) >> 3;
        const int half = threadIdx.x >> 8, tid = threadIdx.x & 255;
        for (int blk = 2 * bx + half; blk < tiles * groups; blk += 2 * PACK_F32_BLOCKS) {
            const int t = blk / groups, g = blk - t * groups;
            const int lane = tid >> 2, i = tid & 3;
            const int row = 32 * t + (lane & 31), col = 8 * g + 2 * i + (lane >> 5);      // row: input feature, col: output feature
            const float v = (row < L.n_in && col < L.n_out) ? weights[L.tensor][(int64_t)col * L.n_in + row] : 0.0f;
            J.stream_f32_t[J.tlayers[layer].frag_off_t + (int64_t)blk * 256 + tid] = v;
        }
        return;
    }
    const int layer = b / PACK_F32_BLOCKS, bx = b - layer * PACK_F32_BLOCKS;
    if (layer >= J.n_layers) return;
    const LayerF32 L = J.layers[layer];
    const int tiles = (L.n_out + 31) >> 5, groups = (L.n_in + 7) >> 3;
    const int half = threadIdx.x >> 8, tid = threadIdx.x & 255;
    for (int blk = 2 * bx + half; blk < tiles * groups; blk += 2 * PACK_F32_BLOCKS) {
        const int t = blk / groups, g = blk - t * groups;
        const int lane = tid >> 2, i = tid & 3;
        const int row = 32 * t + (lane & 31), col = 8 * g + 2 * i + (lane >> 5);
        const float v = (row < L.n_out && col < L.n_in) ? weights[L.tensor][(int64_t)row * L.n_in + col] : 0.0f;
        J.stream_f32[L.frag_off + (int64_t)blk * 256 + tid] = v;
    }
    for (int i = bx * 512 + threadIdx.x; i < tiles * 32; i += PACK_F32_BLOCKS * 512)
        J.bias_f32[L.bias_off + i] = i < L.n_out ? biases[L.tensor][i] : 0.0f;
}

// The fold of feature_linear into views_linears.0 (program.h, ST_S16_FOLD): row o of the FOLD tensor,
//   fold_w[o][i] = sum_k Wv[o][k] Wf[k][i] (i < W),  fold_w[o][W + j] = Wv[o][W + j],  fold_b[o] = sum_k Wv[o][k] bf[k] + bv[o],
// from the fp32 parameters, k ascending in one fp32 fma chain: deterministic, and exact on small-integer weights.
// 8.4 M MAC once per weight change; one block per row.  fold_row is shared with the host twin.
NA_HD inline float fold_dot(const float *wv_row, const float *wf_col, int stride, int W) {
    float acc = 0.0f;
    for (int k = 0; k < W; ++k) acc = __builtin_fmaf(wv_row[k], wf_col[(int64_t)k * stride], acc);
    return acc;
}

__global__ __launch_bounds__(256) void fold_kernel(const float *wf, const float *bf, const float *wv, const float *bv, int W, int n_views,
                                                   float *fold_w, float *fold_b) {
    const int o = blockIdx.x, n_in = W + n_views;
    const float *row = wv + (int64_t)o * n_in;
    for (int i = threadIdx.x; i < n_in; i += blockDim.x)
        fold_w[(int64_t)o * n_in + i] = i < W ? fold_dot(row, wf + i, W, W) : row[i];
    if (threadIdx.x == 0) fold_b[o] = fold_dot(row, bf, 1, W) + bv[o];
}

namespace {
// The jobs of the streams whose copy bit (or, for the bias table, its other reader's) is in `copies`, and their blocks.
PackJobs stream_jobs(const Program &p, const DevTables &t, int copies) {
    PackJobs J{};
    J.tensors = t.d_tensors;
    int blocks = 0;
    for (int i = 0; i < N_STREAMS; ++i) {
        J.frag[i] = {t.st[i].d_frags, t.st[i].stream};
        J.end[i] = blocks += copies & STREAMS[i].copy ? (int)p.streams[i].frags.size() : 0;
    }
    for (int i = 0; i < N_STREAMS; ++i) {
        const bool wanted = copies & (STREAMS[i].copy | STREAMS[i].bias_copy);
        J.bias[i] = {t.st[i].d_tiles, t.st[i].bias, wanted ? (int)p.streams[i].tiles.size() * STREAMS[i].bias_rows : 0, STREAMS[i].bias_rows};
        J.end[N_STREAMS + i] = blocks += (J.bias[i].n + 511) / 512;
    }
    return J;
}

int launch_jobs(const PackJobs &J, const PtrTable &d_w, const PtrTable &d_b, hipStream_t s) {
    const unsigned grid = (unsigned)(J.end[2 * N_STREAMS - 1] + (J.n_layers + J.n_layers_t) * PACK_F32_BLOCKS);
    if (grid == 0) return NERF_AMD_OK;
    hipLaunchKernelGGL(pack_all_kernel, dim3(grid), dim3(512), 0, s, J, d_w, d_b);
    return hipGetLastError() == hipSuccess ? NERF_AMD_OK : NERF_AMD_EHIP;
}
}  // namespace

// The folded stream and its bias table, by launches of their own (a captured training step packs exactly what it always
// packed): the tables' entry p.fold_tensor is the FOLD tensor.
int launch_pack_fold(const Program &p, const DevTables &t, PtrTable d_w, PtrTable d_b, hipStream_t s) {
    if (p.fold_tensor < 0 || p.streams[ST_S16_FOLD].frags.empty()) return NERF_AMD_OK;          // nothing to fold
    if (p.fold_tensor >= MAX_TENSORS) return NERF_AMD_EINVAL;
    const int D = p.arch.D, W = p.arch.W;
    hipLaunchKernelGGL(fold_kernel, dim3(W / 2), dim3(256), 0, s, d_w.p[D], d_b.p[D], d_w.p[D + 2], d_b.p[D + 2], W,
                       p.input_ch_views, t.fold_w, t.fold_b);
    d_w.p[p.fold_tensor] = t.fold_w;
    d_b.p[p.fold_tensor] = t.fold_b;
    return launch_jobs(stream_jobs(p, t, NERF_AMD_COPY_BF16_FOLD), d_w, d_b, s);
}

int launch_pack(const Program &p, const DevTables &t, const PtrTable &d_w, const PtrTable &d_b, int copies, hipStream_t s) {
    PackJobs J = stream_jobs(p, t, copies & ~NERF_AMD_COPY_BF16_FOLD);
    J.layers = t.d_layers; J.tlayers = t.d_tlayers;
    J.stream_f32 = t.stream_f32; J.bias_f32 = t.bias_f32; J.stream_f32_t = t.stream_f32_t;
    J.n_layers = (copies & NERF_AMD_COPY_FP32) ? (int)p.layers.size() : 0;
    J.n_layers_t = (copies & NERF_AMD_COPY_FP32_BWD) && t.stream_f32_t ? (int)p.layers.size() : 0;
    return launch_jobs(J, d_w, d_b, s);
}

void pack_bf16_host(const Program &p, StreamId id, const float *const *w, const float *const *b, uint16_t *stream, float *bias) {
    const FragStream &fs = p.streams[id];
    const TensorDesc *tensors = p.tensors.data();
    std::vector<const float *> ww, bb;       // the tables extended by the FOLD tensor
    std::vector<TensorDesc> td;
    std::vector<float> fw, fb;
    if (id == ST_S16_FOLD) {       // the FOLD tensor first, like fold_kernel
        if (p.fold_tensor < 0) return;
        ww.assign(w, w + p.tensors.size());
        bb.assign(b, b + p.tensors.size());
        td = p.tensors;
        const int D = p.arch.D, W = p.arch.W, n_in = W + p.input_ch_views;
        fw.resize((size_t)(W / 2) * n_in);
        fb.resize(W / 2);
        for (int o = 0; o < W / 2; ++o) {
            const float *row = w[D + 2] + (int64_t)o * n_in;
            for (int i = 0; i < n_in; ++i) fw[(size_t)o * n_in + i] = i < W ? fold_dot(row, w[D] + i, W, W) : row[i];
            fb[o] = fold_dot(row, b[D], 1, W) + b[D + 2][o];
        }
        ww.push_back(fw.data());
        bb.push_back(fb.data());
        td.push_back({W / 2, n_in});
        w = ww.data(); b = bb.data(); tensors = td.data();
    }
    if (stream)
        for (size_t n = 0; n < fs.frags.size(); ++n)
            for (int e = 0; e < 512; ++e) stream[n * 512 + e] = frag_value(fs.frags[n], e >> 3, e & 7, tensors, w);
    const int rows = STREAMS[id].bias_rows;
    if (bias)
        for (size_t e = 0; e < fs.tiles.size() * rows; ++e) bias[e] = bias_value(fs.tiles.data(), rows, (int)e, tensors, b);
}

}  // namespace na
