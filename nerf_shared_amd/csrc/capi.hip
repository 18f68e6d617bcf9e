// capi.hip -- the extern "C" boundary declared in include/nerf_amd.h.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>

#include <cstdio>
#include <cstring>
#include <mutex>
#include <utility>
#include <new>
#include <string>
#include <vector>

#include "kernels.h"
#include "launch_util.h"
#include "program.h"

using namespace na;

namespace {
thread_local std::string g_err;

std::string lds_msg(const char *what, size_t bytes) {
    return std::string(what) + ": the per-ray scratch needs " + std::to_string(bytes) + " bytes of LDS per workgroup, the CU has " +
           std::to_string(LDS_LIMIT_BYTES) + " (fewer samples per ray)";
}

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
int hip_fail(hipError_t e, const char *what) {
    return fail(NERF_AMD_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIP_TRY(expr)                                        \
    do {                                                     \
        hipError_t e_ = (expr);                              \
        if (e_ != hipSuccess) return hip_fail(e_, #expr);    \
    } while (0)

// ---- measurement hook: hipEvent pairs around field launches
struct ProfRec { hipEvent_t a, b; int cls; double points; };
std::mutex g_prof_mu;
bool g_prof_on = false;
std::vector<ProfRec> g_prof_recs;
std::vector<std::pair<hipEvent_t, hipEvent_t>> g_prof_free;

template <class T>
int upload(T **dst, const std::vector<T> &src) {
    *dst = nullptr;
    if (src.empty()) return NERF_AMD_OK;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(dst), src.size() * sizeof(T)));
    HIP_TRY(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return NERF_AMD_OK;
}
size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

// ---- {ticket, done} pairs of the dynamic deal (launch_util.h)
constexpr int TILE_CTR_SLOTS = 1024;
unsigned *g_tile_ctr[16] = {};
std::atomic<unsigned> g_tile_ctr_next{0};
}  // namespace

namespace na {
// tuning knob (nerf_amd_set_tuning key 0): 0 = 16x16x32 kernel, 100+ = the shapes of mlp_bf16.hip (launch_one).  Atomic: the
// launchers of concurrent host threads read it while nerf_amd_set_tuning may write it (nerf_amd.h threading contract).
std::atomic<int> g_variant{0};
// nerf_amd_set_tuning key 2: where bf16 view-branch models run the folded stream (feature_linear folded into views_linears.0):
// 0 the no-grad render path, 1 nowhere, 2 nerf_amd_nerf_forward too
std::atomic<int> g_fold{0};
// nerf_amd_set_tuning key 3: the colour branch of sample blocks without density in the folded render kernels (MlpArgs::view_skip):
// 0 skipped where the render allows it (stage_field), 1 never (the A/B leg: every point runs the full instruction path)
std::atomic<int> g_view_skip_off{0};

int tile_counters_init(int device) {
    if (device < 0 || device >= 16) return NERF_AMD_EINVAL;
    if (g_tile_ctr[device]) return NERF_AMD_OK;
    unsigned *p = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&p), TILE_CTR_SLOTS * 2 * sizeof(unsigned)) != hipSuccess) return NERF_AMD_EHIP;
    if (hipMemset(p, 0, TILE_CTR_SLOTS * 2 * sizeof(unsigned)) != hipSuccess) { (void)hipFree(p); return NERF_AMD_EHIP; }
    g_tile_ctr[device] = p;
    return NERF_AMD_OK;
}

unsigned *tile_counter_slot(int device) {
    if (device < 0 || device >= 16 || !g_tile_ctr[device]) return nullptr;
    return g_tile_ctr[device] + 2 * (g_tile_ctr_next.fetch_add(1, std::memory_order_relaxed) % TILE_CTR_SLOTS);
}

unsigned *tile_counter_for(bool deal, hipStream_t s) {
    if (!deal) return nullptr;
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess || st != hipStreamCaptureStatusNone) return nullptr;
    int dev = 0;
    return hipGetDevice(&dev) == hipSuccess ? tile_counter_slot(dev) : nullptr;
}
}  // namespace na

struct nerf_amd_model : DevTables {
    Program prog;
    int device = 0;
    int fresh = 0;                       // NERF_AMD_COPY_* of the packed copies that hold the current parameters
};

extern "C" {

int nerf_amd_abi_version(void) { return NERF_AMD_ABI_VERSION; }
const char *nerf_amd_last_error(void) { return g_err.c_str(); }

int nerf_amd_model_create(const nerf_amd_arch *arch, int device, nerf_amd_model **out) {
    if (!arch || !out) return fail(NERF_AMD_EINVAL, "null argument");
    *out = nullptr;
    nerf_amd_model *m = new (std::nothrow) nerf_amd_model;
    if (!m) return fail(NERF_AMD_ENOMEM, "out of host memory");
    const char *err = "";
    if (build_program(*arch, m->prog, &err) != 0) {
        delete m;
        return fail(NERF_AMD_EINVAL, err);
    }
    m->device = device;
    if (hipError_t e0 = hipSetDevice(device); e0 != hipSuccess) {
        delete m;
        return hip_fail(e0, "hipSetDevice");
    }
    const Program &p = m->prog;
    int rc;
    std::vector<TensorDesc> tensors_dev(p.tensors);      // + the FOLD tensor at p.fold_tensor (the pack kernels' table only)
    if (p.fold_tensor >= 0) tensors_dev.push_back({p.arch.W / 2, p.arch.W + p.input_ch_views});
    rc = upload(&m->d_layers, p.layers);
    if (!rc) rc = upload(&m->d_tensors, tensors_dev);
    if (!rc) rc = upload(&m->d_tlayers, p.tlayers);
    for (int i = 0; i < N_STREAMS && !rc; ++i)
        if (!(rc = upload(&m->st[i].d_frags, p.streams[i].frags))) rc = upload(&m->st[i].d_tiles, p.streams[i].tiles);
    if (rc) {
        nerf_amd_model_destroy(m);
        return rc;
    }
    // (the streams of a model outside the fused family are empty: nothing is allocated for them)
    hipError_t e = hipSuccess;
    for (int i = 0; i < N_STREAMS && e == hipSuccess; ++i) {
        const FragStream &fs = p.streams[i];
        if (!fs.frags.empty()) e = hipMalloc(reinterpret_cast<void **>(&m->st[i].stream), fs.frags.size() * 1024);
        if (e == hipSuccess && !fs.tiles.empty())
            e = hipMalloc(reinterpret_cast<void **>(&m->st[i].bias), fs.tiles.size() * STREAMS[i].bias_rows * sizeof(float));
    }
    if (e == hipSuccess && m->st[ST_S16_FOLD].stream) {
        const size_t rows = (size_t)p.arch.W / 2, cols = (size_t)p.arch.W + p.input_ch_views;
        e = hipMalloc(reinterpret_cast<void **>(&m->fold_w), rows * cols * sizeof(float));
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&m->fold_b), rows * sizeof(float));
    }
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&m->stream_f32), (size_t)p.f32_stream_floats * sizeof(float));
    if (e == hipSuccess && tile_counters_init(device) != NERF_AMD_OK) e = hipErrorOutOfMemory;      // the field kernel's ticket counters
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&m->bias_f32), (size_t)p.f32_bias_floats * sizeof(float));
    if (e == hipSuccess && p.f32_stream_t_floats > 0)
        e = hipMalloc(reinterpret_cast<void **>(&m->stream_f32_t), (size_t)p.f32_stream_t_floats * sizeof(float));
    if (e != hipSuccess) {
        nerf_amd_model_destroy(m);
        return hip_fail(e, "hipMalloc(model buffers)");
    }
    *out = m;
    return NERF_AMD_OK;
}

int nerf_amd_model_update_copies(nerf_amd_model *m, const float *const *weights, const float *const *biases,
                                 int n_tensors, int copies, int others_current, void *stream) {
    if (!m || !weights || !biases) return fail(NERF_AMD_EINVAL, "null argument");
    if (copies & ~(NERF_AMD_COPY_ALL | NERF_AMD_COPY_BF16_FOLD)) return fail(NERF_AMD_EINVAL, "unknown copy bits");
    const Program &p = m->prog;
    if (n_tensors != (int)p.tensors.size())
        return fail(NERF_AMD_EINVAL, "expected " + std::to_string(p.tensors.size()) + " parameter tensors, got " + std::to_string(n_tensors));
    for (int i = 0; i < n_tensors; ++i)
        if (!weights[i] || !biases[i]) return fail(NERF_AMD_EINVAL, "null parameter pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n_tensors > MAX_TENSORS) return fail(NERF_AMD_EINVAL, "too many parameter tensors");
    PtrTable wt, bt;
    std::memset(&wt, 0, sizeof(wt));
    std::memset(&bt, 0, sizeof(bt));
    for (int i = 0; i < n_tensors; ++i) { wt.p[i] = weights[i]; bt.p[i] = biases[i]; }
    int rc = launch_pack(p, *m, wt, bt, copies, s);
    // the folded stream: launches of its own, only when asked for (a captured training step packs what it always packed)
    if (!rc && (copies & NERF_AMD_COPY_BF16_FOLD) && m->st[ST_S16_FOLD].stream) rc = launch_pack_fold(p, *m, wt, bt, s);
    if (rc) return fail(rc, "pack launch failed");
    m->fresh = (others_current ? m->fresh : 0) | copies;
    return NERF_AMD_OK;
}

int nerf_amd_model_update(nerf_amd_model *m, const float *const *weights, const float *const *biases,
                          int n_tensors, void *stream) {
    return nerf_amd_model_update_copies(m, weights, biases, n_tensors, NERF_AMD_COPY_ALL, 0, stream);
}

void nerf_amd_model_destroy(nerf_amd_model *m) {
    if (!m) return;
    for (DevStream &d : m->st) { (void)hipFree(d.d_frags); (void)hipFree(d.d_tiles); (void)hipFree(d.stream); (void)hipFree(d.bias); }
    (void)hipFree(m->d_layers); (void)hipFree(m->d_tensors); (void)hipFree(m->d_tlayers);
    (void)hipFree(m->stream_f32); (void)hipFree(m->bias_f32); (void)hipFree(m->stream_f32_t);
    (void)hipFree(m->fold_w); (void)hipFree(m->fold_b);
    delete m;
}

int nerf_amd_model_supports_bf16(const nerf_amd_model *m) {
    if (!m) return 0;
    const nerf_amd_arch &a = m->prog.arch;
    return fused_program(m->prog) && mlp_bf16_supported(a.multires, a.multires_views, a.use_viewdirs);
}
int nerf_amd_model_supports_split(const nerf_amd_model *m) {
    if (!m) return 0;
    const nerf_amd_arch &a = m->prog.arch;
    return fused_program(m->prog) && mlp_split_supported(a.multires, a.multires_views, a.use_viewdirs, m->prog.out_ch);
}
int nerf_amd_model_out_ch(const nerf_amd_model *m) { return m ? m->prog.out_ch : 0; }

int nerf_amd_pack_bf16_host(const nerf_amd_arch *arch, int shape, const float *const *weights, const float *const *biases,
                            int n_tensors, uint16_t *stream_out, int64_t *n_frags, float *bias_out, int64_t *n_bias) {
    const int id = stream_of_shape(shape);
    if (id < 0) {
        std::string msg;
        for (const StreamInfo &info : STREAMS)
            msg += (msg.empty() ? "shape must be " : ", ") + std::to_string(info.shape) + " (" + info.what + ")";
        return fail(NERF_AMD_EINVAL, msg);
    }
    if (!arch) return fail(NERF_AMD_EINVAL, "null argument");
    Program p;
    const char *err = "";
    if (build_program(*arch, p, &err) != 0) return fail(NERF_AMD_EINVAL, err);
    if (!p.bf16_ok) return fail(NERF_AMD_EUNSUPPORTED, "architecture has no fused bf16 program (needs D=8, W=256, skips=[4])");
    if (id == ST_S16_FOLD && p.fold_tensor < 0) return fail(NERF_AMD_EUNSUPPORTED, "architecture has no view branch: nothing to fold");
    if (n_frags) *n_frags = (int64_t)p.streams[id].frags.size();
    if (n_bias) *n_bias = (int64_t)p.streams[id].tiles.size() * STREAMS[id].bias_rows;
    if (stream_out || bias_out) {
        if (!weights || !biases || n_tensors != (int)p.tensors.size()) return fail(NERF_AMD_EINVAL, "bad parameter list");
        pack_bf16_host(p, (StreamId)id, weights, biases, stream_out, bias_out);
    }
    return NERF_AMD_OK;
}

int nerf_amd_embed(const float *x, int64_t n, int multires, float *out, void *stream) {
    if (n < 0 || multires < 0 || multires > 20 || (n > 0 && (!x || !out))) return fail(NERF_AMD_EINVAL, "bad embed arguments");
    int rc = launch_embed(x, n, multires, out, static_cast<hipStream_t>(stream));
    return rc ? fail(rc, "embed launch failed") : NERF_AMD_OK;
}

}  // extern "C"

namespace {

// The packed copy an entry point is about to read must hold the current parameters.
int need_copy(const nerf_amd_model *m, int copy) {
    if (m->fresh & copy) return NERF_AMD_OK;
    return fail(NERF_AMD_EINVAL, m->fresh ? "the packed copy of the parameters this call needs is stale or was never made (nerf_amd_model_update_copies)"
                                          : "model has no parameters yet (call nerf_amd_model_update)");
}

// the packed copy a forward pass in `precision` reads
int copy_for(int precision) {
    return precision == NERF_AMD_PREC_BF16 ? NERF_AMD_COPY_BF16 : precision == NERF_AMD_PREC_FP32_SPLIT ? NERF_AMD_COPY_SPLIT : NERF_AMD_COPY_FP32;
}

// The points of a launch: explicit pts [P,3] (+ viewdirs [R,3]), or rays [R,ray_ch] + z_vals [R,S] (view directions at
// column 8 of a ray).  vd: the model has a view branch.
void set_inputs(MlpArgs &a, const float *pts, const float *viewdirs, const float *rays, int ray_ch, const float *z_vals, bool vd) {
    if (pts) { a.pts = pts; a.viewdirs = vd ? viewdirs : nullptr; a.vd_stride = 3; }
    else { a.rays = rays; a.ray_stride = ray_ch; a.z_vals = z_vals; a.viewdirs = vd ? rays + 8 : nullptr; a.vd_stride = ray_ch; }
}

// what the kernels that walk the fp32 program need to know of the model
void set_model_constants(MlpArgs &a, const nerf_amd_model *m) {
    const Program &p = m->prog;
    a.layers = m->d_layers; a.n_layers = (int)p.layers.size();
    a.input_ch = p.input_ch; a.input_ch_views = p.input_ch_views; a.W = p.arch.W; a.lds_rows = p.lds_rows;
    a.multires = p.arch.multires; a.multires_views = p.arch.multires_views; a.i_embed = p.arch.i_embed;
    a.out_ch = p.out_ch;
}

// every packed copy of the parameters, where the kernels look for it
void bind_streams(MlpArgs &a, const nerf_amd_model *m) {
    a.stream_bf16 = m->st[ST_BF16_32].stream; a.bias_bf16 = m->st[ST_BF16_32].bias;
    a.stream_s16 = m->st[ST_S16].stream; a.bias_s16 = m->st[ST_S16].bias;
    a.stream_split = m->st[ST_SPLIT].stream;             // (its bias table is the s16 stream's)
    a.stream_bwd = m->st[ST_BWD].stream; a.stream_bwd_split = m->st[ST_BWD_SPLIT].stream;
    a.stream_f32 = m->stream_f32; a.bias_f32 = m->bias_f32;
}

// fold_mode: what tuning key 2 lets this caller do with the folded stream of a bf16 view-branch model of the fused family
// (16x16x32 kernels).  FOLD_IF_CURRENT (the render path): taken when the folded copy holds the current parameters
// (NERF_AMD_COPY_BF16_FOLD: asked for by whoever renders), else the unfolded stream as always.  FOLD_REQUIRED (key 2 = 2,
// nerf_amd_nerf_forward): a missing copy is an error, so a test of the folded kernel cannot pass on the unfolded one.
enum { FOLD_NEVER = 0, FOLD_IF_CURRENT = 1, FOLD_REQUIRED = 2 };
int run_field(const nerf_amd_model *m, MlpArgs a, int precision, hipStream_t s, int fold_mode = FOLD_NEVER) {
    const Program &p = m->prog;
    const FragStream &s32 = p.streams[ST_BF16_32], &s16 = p.streams[ST_S16], &sfold = p.streams[ST_S16_FOLD];
    if (int rc0 = need_copy(m, copy_for(precision))) return rc0;
    const int variant = g_variant.load(std::memory_order_relaxed);
    const bool foldable = precision == NERF_AMD_PREC_BF16 && m->st[ST_S16_FOLD].stream && nerf_amd_model_supports_bf16(m) &&
                          variant < 100 && variant != 40;      // (40: the round-1 shape of the A/B table has no folded twin)
    if (fold_mode == FOLD_REQUIRED && foldable)
        if (int rc0 = need_copy(m, NERF_AMD_COPY_BF16_FOLD)) return rc0;
    const bool fold = fold_mode != FOLD_NEVER && foldable && (m->fresh & NERF_AMD_COPY_BF16_FOLD);
    bind_streams(a, m);
    set_model_constants(a, m);
    if (p.arch.use_viewdirs && !a.viewdirs) return fail(NERF_AMD_EINVAL, "model has a view branch but no viewdirs were given");
    if (!p.arch.use_viewdirs) a.viewdirs = nullptr;
    int rc;
    ProfRec rec{nullptr, nullptr, precision == NERF_AMD_PREC_BF16 ? 1 : precision == NERF_AMD_PREC_FP32_SPLIT ? 2 : 0, (double)a.P};
    bool prof = false;
    {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        if (g_prof_on) {
            prof = true;
            if (!g_prof_free.empty()) {
                rec.a = g_prof_free.back().first; rec.b = g_prof_free.back().second;
                g_prof_free.pop_back();
            } else if (hipEventCreate(&rec.a) != hipSuccess || hipEventCreate(&rec.b) != hipSuccess) {
                prof = false;
            }
        }
    }
    if (prof) (void)hipEventRecord(rec.a, s);
    struct Closer {
        bool on; ProfRec r; hipStream_t s;
        ~Closer() {
            if (!on) return;
            (void)hipEventRecord(r.b, s);
            std::lock_guard<std::mutex> lk(g_prof_mu);
            g_prof_recs.push_back(r);
        }
    } closer{prof, rec, s};
    if (precision == NERF_AMD_PREC_BF16) {
        if (!nerf_amd_model_supports_bf16(m))
            return fail(NERF_AMD_EUNSUPPORTED, "fused bf16 kernel needs D=8, W=256, skips=[4], multires/views in {(10,4),(15,6)}; use NERF_AMD_PREC_FP32");
        if (g_variant >= 100)   // A/B: the first-generation 32x32x16 kernel
            rc = launch_mlp_bf16(a, p.arch.multires, p.arch.multires_views, p.arch.use_viewdirs, s32.n_used, (int)s32.tiles.size(), s);
        else {
            if (fold) {
                a.stream_s16 = m->st[ST_S16_FOLD].stream; a.bias_s16 = m->st[ST_S16_FOLD].bias;
                rc = launch_mlp_bf16_s16(a, p.arch.multires, p.arch.multires_views, 1, sfold.n_used, (int)sfold.tiles.size(), s, true);
            } else
            rc = launch_mlp_bf16_s16(a, p.arch.multires, p.arch.multires_views, p.arch.use_viewdirs, s16.n_used, (int)s16.tiles.size(), s);
            if (rc == NERF_AMD_EUNSUPPORTED)   // e.g. output_ch > 16: the 32x32x16 kernel covers it
                rc = launch_mlp_bf16(a, p.arch.multires, p.arch.multires_views, p.arch.use_viewdirs, s32.n_used, (int)s32.tiles.size(), s);
        }
    } else if (precision == NERF_AMD_PREC_FP32) {
        rc = launch_mlp_f32(a, s);
    } else if (precision == NERF_AMD_PREC_FP32_SPLIT) {
        if (!nerf_amd_model_supports_split(m))
            return fail(NERF_AMD_EUNSUPPORTED, "split-precision kernel needs D=8, W=256, skips=[4], multires/views in {(10,4),(15,6)} (or 10 / 15 without a view branch, output_ch <= 16); use NERF_AMD_PREC_FP32");
        rc = launch_mlp_split(a, p.arch.multires, p.arch.multires_views, p.arch.use_viewdirs, p.streams[ST_SPLIT].n_used, (int)s16.tiles.size(), s);
    } else {
        return fail(NERF_AMD_EINVAL, "unknown precision");
    }
    return rc ? fail(rc, "field kernel launch failed") : NERF_AMD_OK;
}

}  // namespace

extern "C" {

int nerf_amd_nerf_forward(const nerf_amd_model *m, const float *pts, const float *viewdirs,
                          int64_t n_rays, int32_t n_samples, float *out, int precision, void *stream) {
    if (!m || n_rays < 0 || n_samples < 1) return fail(NERF_AMD_EINVAL, "bad forward arguments");
    if (n_rays == 0) return NERF_AMD_OK;
    if (!pts || !out) return fail(NERF_AMD_EINVAL, "null pts/out");
    MlpArgs a{};
    set_inputs(a, pts, viewdirs, nullptr, 0, nullptr, true);      // (run_field drops viewdirs for a model without view branch)
    a.P = n_rays * n_samples; a.S = n_samples; a.out = out;
    return run_field(m, a, precision, static_cast<hipStream_t>(stream),
                     g_fold.load(std::memory_order_relaxed) == 2 ? FOLD_REQUIRED : FOLD_NEVER);
}

int nerf_amd_mlp_embedded(const nerf_amd_model *m, const float *x, int64_t n, float *out, void *stream) {
    if (!m || n < 0) return fail(NERF_AMD_EINVAL, "bad MLP arguments");
    if (n == 0) return NERF_AMD_OK;
    if (!x || !out) return fail(NERF_AMD_EINVAL, "null x/out");
    MlpArgs a{};
    a.embedded = x;
    a.viewdirs = x;            // non-null marker: the view columns are inside x
    a.vd_stride = 0;
    a.P = n; a.S = 1; a.out = out;
    return run_field(m, a, NERF_AMD_PREC_FP32, static_cast<hipStream_t>(stream));
}

int nerf_amd_ndc_rays(int32_t H, int32_t W, double focal, float near, const float *rays_o, const float *rays_d,
                      int64_t n, float *out_o, float *out_d, void *stream) {
    if (H < 1 || W < 1 || n < 0 || (n > 0 && (!rays_o || !rays_d || !out_o || !out_d)))
        return fail(NERF_AMD_EINVAL, "bad ndc_rays arguments");
    int rc = launch_ndc_rays(H, W, focal, near, rays_o, rays_d, n, out_o, out_d, static_cast<hipStream_t>(stream));
    return rc ? fail(rc, "ndc_rays launch failed") : NERF_AMD_OK;
}

int nerf_amd_ndc_rays_backward(int32_t H, int32_t W, double focal, float near, const float *rays_o, const float *rays_d,
                               const float *g_out_o, const float *g_out_d, int64_t n, float *g_rays_o, float *g_rays_d,
                               void *stream) {
    if (H < 1 || W < 1 || n < 0 || (n > 0 && (!rays_o || !rays_d)))
        return fail(NERF_AMD_EINVAL, "bad ndc_rays_backward arguments");
    int rc = launch_ndc_rays_bwd(H, W, focal, near, rays_o, rays_d, g_out_o, g_out_d, n, g_rays_o, g_rays_d,
                                 static_cast<hipStream_t>(stream));
    return rc ? fail(rc, "ndc_rays backward launch failed") : NERF_AMD_OK;
}

namespace {
const char *TRAIN_COVER = "fused training kernels cover D=8, W=256, skips=[4] with view branch (multires 10/4 or 15/6) or without (multires 10 or 15, output_ch <= 16), in NERF_AMD_PREC_BF16 or NERF_AMD_PREC_FP32_SPLIT; NERF_AMD_PREC_FP32 trains any architecture";
// which training path a (model, precision) pair takes: 1 fused bf16 / split kernels, 2 the exact-fp32 path, 0 none
int train_path(const nerf_amd_model *m, int precision) {
    if ((precision == NERF_AMD_PREC_BF16 || precision == NERF_AMD_PREC_FP32_SPLIT) && train_supported(m->prog)) return 1;
    if (precision == NERF_AMD_PREC_FP32 && train_f32_supported(m->prog)) return 2;
    return 0;
}
// NERF_AMD_SPLIT_TRAIN_MAX_POINTS: dw2s_body (backward.hip) builds the buffer resources of its [pad_points(P), ld <= 256] fp16
// planes and its per-chunk scalar offsets from 32-bit byte counts; one point more and pad_points(P) * 256 * 2 wraps.
static_assert(pad_points(NERF_AMD_SPLIT_TRAIN_MAX_POINTS) * 256 * 2 < ((int64_t)1 << 32) &&
              pad_points(NERF_AMD_SPLIT_TRAIN_MAX_POINTS + 1) * 256 * 2 >= ((int64_t)1 << 32), "split training point limit");
int split_point_limit(int64_t P) {
    if (P <= NERF_AMD_SPLIT_TRAIN_MAX_POINTS) return NERF_AMD_OK;
    return fail(NERF_AMD_EINVAL, "NERF_AMD_PREC_FP32_SPLIT training takes at most NERF_AMD_SPLIT_TRAIN_MAX_POINTS = " +
                std::to_string(NERF_AMD_SPLIT_TRAIN_MAX_POINTS) + " points (2^23 - 256) per call, got R*S = " + std::to_string(P) +
                " (the weight-gradient kernel's 32-bit buffer offsets): split the call into pieces of whole rays");
}
}  // namespace

int nerf_amd_model_supports_training(const nerf_amd_model *m, int precision) {
    return m && train_path(m, precision) ? 1 : 0;
}

int64_t nerf_amd_train_workspace(const nerf_amd_model *m, int64_t n_points, int precision) {
    if (!m || n_points < 0) return -1;
    const int path = train_path(m, precision);
    if (path == 2) return train_f32_workspace_bytes(m->prog, n_points);
    if (path != 1) return -1;
    return train_workspace_bytes(m->prog, n_points, precision == NERF_AMD_PREC_FP32_SPLIT);
}

int nerf_amd_field_forward_train(const nerf_amd_model *m, const float *pts, const float *viewdirs, const float *rays,
                                 int32_t ray_ch, const float *z_vals, int64_t R, int32_t S, float *raw, void *workspace,
                                 int64_t workspace_bytes, int precision, void *stream) {
    if (!m || R < 0 || S < 1) return fail(NERF_AMD_EINVAL, "bad forward_train arguments");
    const bool vd = m->prog.arch.use_viewdirs != 0;
    if (!pts && ray_ch != (vd ? 11 : 8)) return fail(NERF_AMD_EINVAL, vd ? "rays must be [R,11]" : "rays must be [R,8] for a model without view branch");
    if (pts && vd && !viewdirs) return fail(NERF_AMD_EINVAL, "pts mode needs viewdirs [R,3]");
    const int path = train_path(m, precision);
    if (!path) return fail(NERF_AMD_EUNSUPPORTED, TRAIN_COVER);
    if (path == 2) {                                   // exact fp32, any architecture (train_f32.hip)
        if (int rc0 = need_copy(m, NERF_AMD_COPY_FP32)) return rc0;
        if (R == 0) return NERF_AMD_OK;
        const int64_t P = R * S;
        if ((!pts && (!rays || !z_vals)) || !raw || !workspace || workspace_bytes < train_f32_workspace_bytes(m->prog, P))
            return fail(NERF_AMD_EINVAL, "null pointer or workspace too small");
        MlpArgs a{};
        bind_streams(a, m);
        set_model_constants(a, m);
        set_inputs(a, pts, viewdirs, rays, ray_ch, z_vals, vd);
        a.P = P; a.S = S; a.out = raw;
        int rc = launch_train_f32_forward(m->prog, a, m->d_tlayers, workspace, static_cast<hipStream_t>(stream));
        return rc ? fail(rc, "exact-fp32 training forward launch failed") : NERF_AMD_OK;
    }
    if (int rc0 = need_copy(m, copy_for(precision))) return rc0;
    if (R == 0) return NERF_AMD_OK;
    const bool split = precision == NERF_AMD_PREC_FP32_SPLIT;
    const int64_t P = R * S;
    if (int rc0 = split ? split_point_limit(P) : NERF_AMD_OK) return rc0;
    if ((!pts && (!rays || !z_vals)) || !raw || !workspace || workspace_bytes < train_workspace_bytes(m->prog, P, split))
        return fail(NERF_AMD_EINVAL, "null pointer or workspace too small");
    MlpArgs a{};
    bind_streams(a, m);
    set_inputs(a, pts, viewdirs, rays, ray_ch, z_vals, vd);
    a.P = P; a.S = S; a.out = raw; a.out_ch = m->prog.out_ch;
    train_fill_args(m->prog, P, workspace, &a, split);
    const nerf_amd_arch &ar = m->prog.arch;
    const FragStream &fs = m->prog.streams[split ? ST_SPLIT : ST_S16];
    const int n_tiles = (int)m->prog.streams[ST_S16].tiles.size();
    int rc = split ? launch_mlp_split_save(a, ar.multires, ar.multires_views, vd, fs.n_used, n_tiles, static_cast<hipStream_t>(stream))
                   : launch_mlp_bf16_s16_save(a, ar.multires, ar.multires_views, vd, fs.n_used, n_tiles, static_cast<hipStream_t>(stream));
    return rc ? fail(rc, "training forward launch failed") : NERF_AMD_OK;
}

// nerf_amd_field_backward (with_params: dX chain, then the weight-gradient products into grad_weights / grad_biases) and
// nerf_amd_field_backward_inputs (the dX chain alone; no tables) are one function: the same checks, the same dX launch.
static int field_backward(const nerf_amd_model *m, const float *g_raw, const float *pts, const float *viewdirs,
                   const float *rays, int32_t ray_ch, const float *z_vals, int64_t R, int32_t S,
                   void *workspace, int64_t workspace_bytes, bool with_params, float *const *grad_weights,
                   float *const *grad_biases, int n_tensors, float *g_pts, float *g_rays, float *g_viewdirs,
                   int precision, void *stream) {
    const int64_t n_points = R * S;
    if (!m || R < 0 || S < 1 || (with_params && (!grad_weights || !grad_biases))) return fail(NERF_AMD_EINVAL, "bad backward arguments");
    const bool vd = m->prog.arch.use_viewdirs != 0;
    if ((!pts && (ray_ch != (vd ? 11 : 8) || !rays || !z_vals)) || (pts && vd && !viewdirs))
        return fail(NERF_AMD_EINVAL, "backward needs the forward's inputs (pts + viewdirs, or rays [R,11] + z_vals; [R,8] without view branch)");
    const int path = train_path(m, precision);
    if (!path) return fail(NERF_AMD_EUNSUPPORTED, TRAIN_COVER);
    if (with_params && n_tensors != (int)m->prog.tensors.size()) return fail(NERF_AMD_EINVAL, "wrong number of gradient tensors");
    if (n_points == 0) return NERF_AMD_OK;
    if (path == 2) {                                   // exact fp32, any architecture (train_f32.hip)
        if (int rc0 = need_copy(m, NERF_AMD_COPY_FP32_BWD)) return rc0;
        if (!g_raw || !workspace || workspace_bytes < train_f32_workspace_bytes(m->prog, n_points))
            return fail(NERF_AMD_EINVAL, "null pointer or workspace too small");
        for (int i = 0; with_params && i < n_tensors; ++i)
            if (!grad_weights[i] || !grad_biases[i]) return fail(NERF_AMD_EINVAL, "null gradient pointer");
        MlpArgs a{};
        set_model_constants(a, m);
        set_inputs(a, pts, viewdirs, rays, ray_ch, z_vals, vd);
        a.g_pts = g_pts; a.g_rays = g_rays; a.g_vd = vd ? g_viewdirs : nullptr;
        a.P = n_points; a.S = S; a.g_raw = g_raw;
        // (the dW / db products of this path are launches of their own after the dX chain: without tables they are skipped)
        int rc = launch_train_f32_backward(m->prog, a, m->d_tlayers, m->stream_f32_t, workspace, with_params ? grad_weights : nullptr,
                                           with_params ? grad_biases : nullptr, static_cast<hipStream_t>(stream));
        return rc ? fail(rc, "exact-fp32 backward launch failed") : NERF_AMD_OK;
    }
    const bool split = precision == NERF_AMD_PREC_FP32_SPLIT;
    if (int rc0 = need_copy(m, split ? NERF_AMD_COPY_BWD_SPLIT : NERF_AMD_COPY_BWD)) return rc0;
    if (int rc0 = split ? split_point_limit(n_points) : NERF_AMD_OK) return rc0;
    if (!g_raw || !workspace || workspace_bytes < train_workspace_bytes(m->prog, n_points, split))
        return fail(NERF_AMD_EINVAL, "null pointer or workspace too small");
    hipStream_t s = static_cast<hipStream_t>(stream);
    MlpArgs a{};
    bind_streams(a, m);
    a.g_raw = g_raw; a.P = n_points; a.S = S; a.out_ch = m->prog.out_ch;
    set_inputs(a, pts, viewdirs, rays, ray_ch, z_vals, vd);
    a.g_pts = g_pts; a.g_rays = g_rays; a.g_vd = vd ? g_viewdirs : nullptr;
    train_fill_args(m->prog, n_points, workspace, &a, split);
    const nerf_amd_arch &ar = m->prog.arch;
    int rc = split ? launch_mlp_bwd_split(a, ar.multires, ar.multires_views, vd, m->prog.streams[ST_BWD_SPLIT].n_used, s)
                   : launch_mlp_bwd_s16(a, ar.multires, ar.multires_views, vd, m->prog.streams[ST_BWD].n_used, s);
    if (rc) return fail(rc, "backward kernel launch failed");
    if (!with_params) return NERF_AMD_OK;
    rc = train_param_grads(m->prog, n_points, workspace, grad_weights, grad_biases, m->device, s, split, g_raw);
    return rc ? fail(rc, "weight-gradient GEMMs failed") : NERF_AMD_OK;
}

int nerf_amd_field_backward(const nerf_amd_model *m, const float *g_raw, const float *pts, const float *viewdirs,
                            const float *rays, int32_t ray_ch, const float *z_vals, int64_t R, int32_t S,
                            void *workspace, int64_t workspace_bytes, float *const *grad_weights,
                            float *const *grad_biases, int n_tensors, float *g_pts, float *g_rays, float *g_viewdirs,
                            int precision, void *stream) {
    return field_backward(m, g_raw, pts, viewdirs, rays, ray_ch, z_vals, R, S, workspace, workspace_bytes, true, grad_weights,
                          grad_biases, n_tensors, g_pts, g_rays, g_viewdirs, precision, stream);
}

int nerf_amd_field_backward_inputs(const nerf_amd_model *m, const float *g_raw, const float *pts, const float *viewdirs,
                                   const float *rays, int32_t ray_ch, const float *z_vals, int64_t R, int32_t S,
                                   void *workspace, int64_t workspace_bytes, float *g_pts, float *g_rays, float *g_viewdirs,
                                   int precision, void *stream) {
    return field_backward(m, g_raw, pts, viewdirs, rays, ray_ch, z_vals, R, S, workspace, workspace_bytes, false, nullptr,
                          nullptr, 0, g_pts, g_rays, g_viewdirs, precision, stream);
}

// ---- density queries (NeRF.get_density, nerf.py:136-143): sigma of a model without view branch, and its gradient
int nerf_amd_density_arch(const nerf_amd_arch *in, nerf_amd_arch *out) {
    if (!in || !out) return fail(NERF_AMD_EINVAL, "null argument");
    nerf_amd_arch t = *in;
    t.use_viewdirs = 0; t.output_ch = 1; t.multires_views = 0;
    Program p;
    const char *err = "";
    if (build_program(t, p, &err) != 0) return fail(NERF_AMD_EINVAL, err);
    *out = t;
    return NERF_AMD_OK;
}

namespace {
std::atomic<int> g_density_route{0};       // nerf_amd_set_tuning key 1: 0 the fused kernel where it covers the model, 1 always two launches
const char *NO_VIEW_BRANCH = "density entry points take a model WITHOUT view branch (the density twin of nerf_amd_density_arch, or an output_linear model)";

bool density_fused_covers(const nerf_amd_model *m, int precision) {
    const nerf_amd_arch &a = m->prog.arch;
    return precision == NERF_AMD_PREC_BF16 && fused_program(m->prog) && !m->prog.streams[ST_BWD].frags.empty() &&
           density_grad_fused_supported(a.multires, a.use_viewdirs, m->prog.out_ch);
}
bool density_takes_fused(const nerf_amd_model *m, int precision) {
    // (the fused kernel is the default because it is the faster route wherever it runs: DESIGN.md section 8d)
    return g_density_route.load(std::memory_order_relaxed) == 0 && density_fused_covers(m, precision);
}
// two-launch route: [training workspace | raw [n, out_ch] | dL/draw [n, out_ch]] (the last two only where they are needed:
// with one channel raw IS sigma)
struct DensityWs { int64_t train, raw, total; };
bool density_ws(const nerf_amd_model *m, int64_t n, int precision, DensityWs *w) {
    const int64_t t = nerf_amd_train_workspace(m, n, precision);
    if (t < 0) return false;
    const int och = m->prog.out_ch;
    w->train = (int64_t)align_up((size_t)t);
    w->raw = och > 1 ? (int64_t)align_up((size_t)n * och * sizeof(float)) : 0;
    w->total = w->train + w->raw + (int64_t)align_up((size_t)n * och * sizeof(float));
    return true;
}
}  // namespace

int nerf_amd_density(const nerf_amd_model *m, const float *pts, int64_t n, float *sigma, int precision, void *stream) {
    if (!m || n < 0) return fail(NERF_AMD_EINVAL, "bad density arguments");
    if (m->prog.arch.use_viewdirs) return fail(NERF_AMD_EINVAL, NO_VIEW_BRANCH);
    if (precision != NERF_AMD_PREC_BF16 && precision != NERF_AMD_PREC_FP32_SPLIT && precision != NERF_AMD_PREC_FP32)
        return fail(NERF_AMD_EINVAL, "unknown precision");
    if (int rc0 = need_copy(m, copy_for(precision))) return rc0;
    if (n == 0) return NERF_AMD_OK;
    if (!pts || !sigma) return fail(NERF_AMD_EINVAL, "null pts/sigma");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int och = m->prog.out_ch;
    MlpArgs a{};
    set_inputs(a, pts, nullptr, nullptr, 0, nullptr, false);
    a.P = n; a.S = 1;
    if (och == 1) {                 // the field kernel's own store is sigma [n]
        a.out = sigma;
        return run_field(m, a, precision, s);
    }
    // more channels: the rows go to stream-ordered scratch and the last column is copied out
    float *raw = nullptr;
    HIP_TRY(hipMallocAsync(reinterpret_cast<void **>(&raw), (size_t)n * och * sizeof(float), s));
    a.out = raw;
    int rc = run_field(m, a, precision, s);
    if (!rc && (rc = launch_density_last_channel(raw, n, och, sigma, s))) fail(rc, "density channel copy launch failed");
    (void)hipFreeAsync(raw, s);
    return rc;
}

int nerf_amd_density_grad_fused(const nerf_amd_model *m, int precision) {
    return m && !m->prog.arch.use_viewdirs && density_takes_fused(m, precision) ? 1 : 0;
}

int64_t nerf_amd_density_grad_workspace(const nerf_amd_model *m, int64_t n, int precision) {
    if (!m || n < 0 || m->prog.arch.use_viewdirs) return -1;
    if (density_takes_fused(m, precision)) return 0;
    DensityWs w;
    return density_ws(m, n, precision, &w) ? w.total : -1;
}

int nerf_amd_density_value_grad(const nerf_amd_model *m, const float *pts, int64_t n, float *sigma, float *grad,
                                void *workspace, int64_t workspace_bytes, int precision, void *stream) {
    if (!m || n < 0) return fail(NERF_AMD_EINVAL, "bad density_value_grad arguments");
    if (m->prog.arch.use_viewdirs) return fail(NERF_AMD_EINVAL, NO_VIEW_BRANCH);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int och = m->prog.out_ch;
    if (density_takes_fused(m, precision)) {
        if (int rc0 = need_copy(m, NERF_AMD_COPY_BF16)) return rc0;
        if (int rc0 = need_copy(m, NERF_AMD_COPY_BWD)) return rc0;
        if (n == 0) return NERF_AMD_OK;
        if (!pts || !sigma || !grad) return fail(NERF_AMD_EINVAL, "null pts/sigma/grad");
        MlpArgs a{};
        bind_streams(a, m);
        a.pts = pts; a.P = n; a.S = 1; a.out = sigma; a.out_ch = och; a.g_pts = grad;
        int rc = launch_density_grad(a, m->prog.arch.multires, m->prog.streams[ST_S16].n_used, (int)m->prog.streams[ST_S16].tiles.size(), m->prog.streams[ST_BWD].n_used, s);
        return rc ? fail(rc, "fused density kernel launch failed") : NERF_AMD_OK;
    }
    // two launches: the training forward (saves the activations), then the dX chain alone with dL/draw = 1 in the sigma column
    const int path = train_path(m, precision);
    if (!path) return fail(NERF_AMD_EUNSUPPORTED, TRAIN_COVER);
    const int fwd_copy = copy_for(precision);
    const int bwd_copy = path == 2 ? NERF_AMD_COPY_FP32_BWD : precision == NERF_AMD_PREC_FP32_SPLIT ? NERF_AMD_COPY_BWD_SPLIT : NERF_AMD_COPY_BWD;
    if (int rc0 = need_copy(m, fwd_copy)) return rc0;
    if (int rc0 = need_copy(m, bwd_copy)) return rc0;
    if (n == 0) return NERF_AMD_OK;
    if (!pts || !sigma || !grad) return fail(NERF_AMD_EINVAL, "null pts/sigma/grad");
    DensityWs w;
    if (!density_ws(m, n, precision, &w)) return fail(NERF_AMD_EUNSUPPORTED, TRAIN_COVER);
    if (!workspace || workspace_bytes < w.total || (reinterpret_cast<uintptr_t>(workspace) & 255))
        return fail(NERF_AMD_EINVAL, "workspace missing, misaligned or too small (nerf_amd_density_grad_workspace bytes, 256-B aligned)");
    char *base = static_cast<char *>(workspace);
    float *raw = och > 1 ? reinterpret_cast<float *>(base + w.train) : sigma;
    float *g_raw = reinterpret_cast<float *>(base + w.train + w.raw);
    int rc = nerf_amd_field_forward_train(m, pts, nullptr, nullptr, 0, nullptr, n, 1, raw, workspace, w.train, precision, stream);
    if (rc) return rc;
    if (och > 1 && (rc = launch_density_last_channel(raw, n, och, sigma, s))) return fail(rc, "density channel copy launch failed");
    if ((rc = launch_density_unit_grad(g_raw, n, och, s))) return fail(rc, "density unit-gradient launch failed");
    return nerf_amd_field_backward_inputs(m, g_raw, pts, nullptr, nullptr, 0, nullptr, n, 1, workspace, w.train, grad, nullptr, nullptr,
                                          precision, stream);
}

int nerf_amd_raw2outputs(const float *raw, int32_t raw_ch, const float *z_vals, const float *rays_d,
                         int32_t rays_d_stride, const float *noise, int64_t R, int32_t S, int white_bkgd,
                         float *rgb_map, float *disp_map, float *acc_map, float *weights, float *depth_map,
                         void *stream) {
    if (R < 0 || S < 1 || raw_ch < 4 || (R > 0 && (!raw || !z_vals || !rays_d))) return fail(NERF_AMD_EINVAL, "bad raw2outputs arguments");
    int rc = launch_composite(raw, raw_ch, z_vals, rays_d, rays_d_stride, noise, R, S, white_bkgd, rgb_map, disp_map,
                              acc_map, weights, depth_map, static_cast<hipStream_t>(stream));
    return rc ? fail(rc, "composite launch failed") : NERF_AMD_OK;
}

int nerf_amd_raw2outputs_backward(const float *raw, int32_t raw_ch, const float *z_vals, const float *rays_d,
                                  int32_t rays_d_stride, const float *noise, int64_t R, int32_t S, int white_bkgd,
                                  const float *g_rgb_map, const float *g_disp_map, const float *g_acc_map,
                                  const float *g_depth_map, const float *g_weights, float *g_raw, float *g_rays_d,
                                  void *stream) {
    if (R < 0 || S < 1 || raw_ch < 4 || (R > 0 && (!raw || !z_vals || !rays_d || !g_raw)))
        return fail(NERF_AMD_EINVAL, "bad raw2outputs_backward arguments");
    int rc = launch_composite_bwd(raw, raw_ch, z_vals, rays_d, rays_d_stride, noise, R, S, white_bkgd, g_rgb_map,
                                  g_disp_map, g_acc_map, g_depth_map, g_weights, g_raw, g_rays_d,
                                  static_cast<hipStream_t>(stream));
    if (rc == NERF_AMD_EINVAL && composite_bwd_lds_bytes(S) > LDS_LIMIT_BYTES) return fail(rc, lds_msg("raw2outputs_backward", composite_bwd_lds_bytes(S)));
    return rc ? fail(rc, "composite backward launch failed") : NERF_AMD_OK;
}

int nerf_amd_sample_pdf(const float *bins, const float *weights, const float *u, const float *t_lin,
                        int64_t R, int32_t n_bins, int32_t n_samples, float *samples, void *stream) {
    if (R < 0 || n_bins < 2 || n_samples < 0 || (R > 0 && (!bins || !weights || !samples || (!u && !t_lin))))
        return fail(NERF_AMD_EINVAL, "bad sample_pdf arguments");
    int rc = launch_sample_pdf(bins, weights, u, t_lin, R, n_bins, n_samples, samples, static_cast<hipStream_t>(stream));
    if (rc == NERF_AMD_EINVAL && sample_pdf_lds_bytes(n_bins) > LDS_LIMIT_BYTES) return fail(rc, lds_msg("sample_pdf", sample_pdf_lds_bytes(n_bins)));
    return rc ? fail(rc, "sample_pdf launch failed") : NERF_AMD_OK;
}

int nerf_amd_coarse_z(const float *rays, int32_t ray_ch, const float *t_vals, const float *t_rand, int64_t R,
                      int32_t N_samples, int lindisp, int perturb, float *z_vals, void *stream) {
    if (R < 0 || N_samples < 1 || ray_ch < 8 || (R > 0 && (!rays || !t_vals || !z_vals || (perturb && !t_rand))))
        return fail(NERF_AMD_EINVAL, "bad coarse_z arguments");
    int rc = launch_coarse_z(rays, ray_ch, t_vals, perturb ? t_rand : nullptr, R, N_samples, lindisp, perturb, z_vals,
                             static_cast<hipStream_t>(stream));
    return rc ? fail(rc, "coarse_z launch failed") : NERF_AMD_OK;
}

int nerf_amd_resample(const float *z_coarse, const float *weights, const float *u, const float *t_lin, int64_t R,
                      int32_t N_samples, int32_t N_importance, float *z_fine, float *z_std, void *stream) {
    if (R < 0 || N_samples < 3 || N_importance < 1 || (R > 0 && (!z_coarse || !weights || !z_fine || (!u && !t_lin))))
        return fail(NERF_AMD_EINVAL, "bad resample arguments");
    int rc = launch_resample(z_coarse, weights, u, t_lin, R, N_samples, N_importance, z_fine, z_std,
                             static_cast<hipStream_t>(stream));
    if (rc == NERF_AMD_EINVAL && resample_lds_bytes(N_samples, N_importance, false) > LDS_LIMIT_BYTES)
        return fail(rc, lds_msg("resample", resample_lds_bytes(N_samples, N_importance, false)));
    return rc ? fail(rc, "resample launch failed") : NERF_AMD_OK;
}

}  // extern "C"

// ---- render_rays over one chunk's buffers, in stages: z_vals, coarse field, coarse compositing (+ resampling),
// fine field, final compositing.  nerf_amd_render_chunks interleaves the stages of consecutive chunks.
namespace {
struct ChunkPlan {
    const nerf_amd_render_cfg *cfg;
    const nerf_amd_model *coarse, *fm;
    const nerf_amd_render_io *io;
    int64_t R;
    int Nc, Ni, Nf, och;
    bool has_vd;
    float *z_c, *raw_c, *w_c, *z_f, *raw_f;
};

// The workspace of one render_rays call, stated once: z / raw / weights of the coarse pass, then with a fine pass its z / raw.
// Counts the bytes (nerf_amd_render_rays_workspace); with `p` and `base` it also carves them (plan_chunk).
size_t rays_ws_bytes(int64_t R, size_t Nc, size_t Ni, size_t och, ChunkPlan *p, char *base) {
    size_t b = 0;
    auto take = [&](size_t bytes) { float *q = base ? reinterpret_cast<float *>(base + b) : nullptr; b += align_up(bytes); return q; };
    const size_t Nf = Nc + Ni;
    float *z_c = take(R * Nc * sizeof(float)), *raw_c = take(R * Nc * och * sizeof(float)), *w_c = take(R * Nc * sizeof(float));
    float *z_f = Ni ? take(R * Nf * sizeof(float)) : nullptr, *raw_f = Ni ? take(R * Nf * och * sizeof(float)) : nullptr;
    if (p) { p->z_c = z_c; p->raw_c = raw_c; p->w_c = w_c; p->z_f = z_f; p->raw_f = raw_f; }
    return b;
}

int plan_chunk(const nerf_amd_render_cfg *cfg, const nerf_amd_model *coarse, const nerf_amd_model *fine,
               const nerf_amd_render_io *io, int64_t R, ChunkPlan *p) {
    if (!cfg || !coarse || !io || R < 0) return fail(NERF_AMD_EINVAL, "null argument");
    const int Nc = cfg->N_samples, Ni = cfg->N_importance, Nf = Nc + Ni;
    if (Nc < 1 || Ni < 0) return fail(NERF_AMD_EINVAL, "bad sample counts");
    // fewer than three coarse samples leave sample_pdf without an interior weight: the reference's cdf is then EMPTY
    // (zeros_like(cdf[..., :1]) of an empty cumsum, utils.py:78-79) and its gather raises an index error
    if (Ni > 0 && Nc < 3) return fail(NERF_AMD_EINVAL, "hierarchical sampling needs N_samples >= 3 (with fewer the reference's sample_pdf fails too: empty cdf)");
    if (Ni > 0 && resample_lds_bytes(Nc, Ni, true) > LDS_LIMIT_BYTES)      // refuse before anything is launched
        return fail(NERF_AMD_EINVAL, lds_msg("render_rays (compositing + resampling)", resample_lds_bytes(Nc, Ni, true)));
    if (!io->rays || (io->ray_ch != 8 && io->ray_ch != 11)) return fail(NERF_AMD_EINVAL, "rays must be [R,8] or [R,11]");
    if (!io->t_vals) return fail(NERF_AMD_EINVAL, "t_vals missing");
    if (cfg->perturb && !io->t_rand && !io->z_coarse) return fail(NERF_AMD_EINVAL, "perturb set but t_rand missing");
    if (cfg->use_noise && (!io->noise0 || (Ni > 0 && !io->noise1))) return fail(NERF_AMD_EINVAL, "use_noise set but noise missing");
    if (Ni > 0 && !io->u && !io->t_lin_imp) return fail(NERF_AMD_EINVAL, "need u or t_lin_imp for sample_pdf");
    const nerf_amd_model *fm = fine ? fine : coarse;
    const int och = coarse->prog.out_ch;
    if (Ni > 0 && fm->prog.out_ch != och) return fail(NERF_AMD_EINVAL, "coarse and fine models disagree on output channels");
    if (och < 4) return fail(NERF_AMD_EINVAL, "field must output at least 4 channels");
    const bool has_vd = io->ray_ch > 8;
    if ((coarse->prog.arch.use_viewdirs != 0) != has_vd || (fm->prog.arch.use_viewdirs != 0) != has_vd)
        return fail(NERF_AMD_EINVAL, "ray batch width does not match the models' use_viewdirs");
    if (io->workspace_bytes < (int64_t)rays_ws_bytes(R, Nc, Ni, och, nullptr, nullptr) || !io->workspace)
        return fail(NERF_AMD_EINVAL, "workspace too small");
    p->cfg = cfg; p->coarse = coarse; p->fm = fm; p->io = io; p->R = R;
    p->Nc = Nc; p->Ni = Ni; p->Nf = Nf; p->och = och; p->has_vd = has_vd;
    rays_ws_bytes(R, Nc, Ni, och, p, static_cast<char *>(io->workspace));
    if (Ni > 0) {      // what the caller wants back is written in place
        if (io->z_vals) p->z_f = io->z_vals;
        if (io->raw) p->raw_f = io->raw;
    } else {
        if (io->z_vals) p->z_c = io->z_vals;
        if (io->raw) p->raw_c = io->raw;
        if (io->weights) p->w_c = io->weights;
    }
    return NERF_AMD_OK;
}

int stage_z(ChunkPlan &p, hipStream_t s) {
    const nerf_amd_render_io *io = p.io;
    int rc = 0;
    if (io->z_coarse) {
        if (p.Ni == 0 && io->z_vals)      // the caller wants z_vals back: they are its own coarse depths
            rc = hipMemcpyAsync(io->z_vals, io->z_coarse, p.R * p.Nc * sizeof(float), hipMemcpyDeviceToDevice, s) == hipSuccess
                     ? 0 : NERF_AMD_EHIP;
        else
            p.z_c = const_cast<float *>(io->z_coarse);
    } else {
        rc = launch_coarse_z(io->rays, io->ray_ch, io->t_vals, p.cfg->perturb ? io->t_rand : nullptr, p.R, p.Nc,
                             p.cfg->lindisp, p.cfg->perturb, p.z_c, s);
    }
    return rc ? fail(rc, "coarse_z launch failed") : NERF_AMD_OK;
}

// the no-grad render path's choice of weight stream (stage_field, field_points): the folded one unless tuning forbids it
int fold_wanted() { return g_fold.load(std::memory_order_relaxed) != 1 ? FOLD_IF_CURRENT : FOLD_NEVER; }

int stage_field(const ChunkPlan &p, bool fine_pass, hipStream_t s) {
    MlpArgs a{};
    set_inputs(a, nullptr, nullptr, p.io->rays, p.io->ray_ch, fine_pass ? p.z_f : p.z_c, p.has_vd);
    a.S = fine_pass ? p.Nf : p.Nc; a.P = p.R * (int64_t)a.S; a.out = fine_pass ? p.raw_f : p.raw_c;
    // raw2outputs gives a sample with sigma <= 0 the weight 1 - exp(-0) = 0 exactly, so its rgb reaches every map as + 0 whatever
    // (finite) value it has -- unless the caller gets raw itself, or noise is added to sigma first (sigma + noise has its own sign)
    a.view_skip = !p.io->raw && !p.cfg->use_noise && !p.io->noise0 && !p.io->noise1 &&
                  g_view_skip_off.load(std::memory_order_relaxed) == 0;
    return run_field(fine_pass ? p.fm : p.coarse, a, p.cfg->precision, s, fold_wanted());
}

CompositeJob final_job(const ChunkPlan &p) {       // compositing of the last pass of a chunk
    const nerf_amd_render_io *io = p.io;
    CompositeJob j;
    std::memset(&j, 0, sizeof(j));
    const bool two_pass = p.Ni > 0;
    j.raw = two_pass ? p.raw_f : p.raw_c; j.raw_ch = p.och; j.z = two_pass ? p.z_f : p.z_c;
    j.rays_d = io->rays + 3; j.rays_d_stride = io->ray_ch;
    j.noise = p.cfg->use_noise ? (two_pass ? io->noise1 : io->noise0) : nullptr;
    j.R = p.R; j.S = two_pass ? p.Nf : p.Nc; j.white_bkgd = p.cfg->white_bkgd;
    j.rgb = io->rgb_map; j.disp = io->disp_map; j.acc = io->acc_map; j.weights = two_pass ? io->weights : p.w_c;
    return j;
}

int stage_final(const ChunkPlan &p, hipStream_t s) {
    const CompositeJob j = final_job(p);
    int rc = launch_composite(j.raw, j.raw_ch, j.z, j.rays_d, j.rays_d_stride, j.noise, j.R, j.S, j.white_bkgd, j.rgb, j.disp,
                              j.acc, j.weights, nullptr, s);
    return rc ? fail(rc, "composite launch failed") : NERF_AMD_OK;
}

// coarse compositing + resampling of `p` (N_importance > 0), together with the final compositing of `prev` if given
int stage_mid(const ChunkPlan &p, const ChunkPlan *prev, hipStream_t s) {
    const nerf_amd_render_io *io = p.io;
    CompositeJob cj;
    std::memset(&cj, 0, sizeof(cj));
    cj.raw = p.raw_c; cj.raw_ch = p.och; cj.z = p.z_c; cj.rays_d = io->rays + 3; cj.rays_d_stride = io->ray_ch;
    cj.noise = p.cfg->use_noise ? io->noise0 : nullptr; cj.R = p.R; cj.S = p.Nc; cj.white_bkgd = p.cfg->white_bkgd;
    cj.rgb = io->rgb0; cj.disp = io->disp0; cj.acc = io->acc0; cj.weights = nullptr;
    ResampleJob rj;
    std::memset(&rj, 0, sizeof(rj));
    rj.u = io->u; rj.t_lin = io->t_lin_imp; rj.Ni = p.Ni; rj.z_fine = p.z_f; rj.z_std = io->z_std;
    CompositeJob fj;
    if (prev) fj = final_job(*prev);
    int rc = launch_mid_stage(cj, rj, prev ? &fj : nullptr, s);
    if (rc == NERF_AMD_EINVAL && resample_lds_bytes(p.Nc, p.Ni, true) > LDS_LIMIT_BYTES)
        return fail(rc, lds_msg("render_rays (compositing + resampling)", resample_lds_bytes(p.Nc, p.Ni, true)));
    return rc ? fail(rc, "composite/resample launch failed") : NERF_AMD_OK;
}

// The stage order, walked once for every entry that runs its chunks one after the other on one stream: per chunk z, coarse
// field, then either the final compositing (no fine pass) or mid and fine field -- with the final compositing of chunk k-1
// folded into chunk k's mid launch, and the last chunk's as a launch of its own.  `field(plan, fine_pass, s)` is the field
// stage: stage_field, or the culled one.  One plan: mid, fine field and final are three launches.
template <class FieldStage>
int walk_chunks(ChunkPlan *plans, int n, FieldStage field, hipStream_t s) {
    int rc = 0;
    for (int k = 0; k < n && !rc; ++k) {
        ChunkPlan &p = plans[k];
        if ((rc = stage_z(p, s)) || (rc = field(p, false, s))) break;
        if (p.Ni == 0) { rc = stage_final(p, s); continue; }
        if ((rc = stage_mid(p, k > 0 ? &plans[k - 1] : nullptr, s))) break;
        rc = field(p, true, s);
    }
    if (!rc && n > 0 && plans[n - 1].Ni > 0) rc = stage_final(plans[n - 1], s);
    return rc;
}
}  // namespace

extern "C" {

int64_t nerf_amd_render_rays_workspace(const nerf_amd_render_cfg *cfg, int64_t R, int32_t out_ch) {
    if (!cfg || R < 0) return -1;
    return (int64_t)rays_ws_bytes(R, cfg->N_samples, cfg->N_importance > 0 ? cfg->N_importance : 0, out_ch, nullptr, nullptr);
}

int nerf_amd_render_rays(const nerf_amd_render_cfg *cfg, const nerf_amd_model *coarse, const nerf_amd_model *fine,
                         const nerf_amd_render_io *io, int64_t R, void *stream) {
    if (R == 0 && cfg && coarse && io) return NERF_AMD_OK;
    ChunkPlan p;
    if (int rc = plan_chunk(cfg, coarse, fine, io, R, &p)) return rc;
    return walk_chunks(&p, 1, stage_field, static_cast<hipStream_t>(stream));
}

int nerf_amd_render_chunks(const nerf_amd_render_cfg *cfg, const nerf_amd_model *coarse, const nerf_amd_model *fine,
                           const nerf_amd_render_io *ios, const int64_t *R, int32_t n_chunks, void *stream) {
    if (n_chunks < 0 || (n_chunks > 0 && (!ios || !R))) return fail(NERF_AMD_EINVAL, "bad chunk list");
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<ChunkPlan> plans;
    plans.reserve(n_chunks);
    for (int i = 0; i < n_chunks; ++i) {
        if (R[i] <= 0) continue;
        ChunkPlan p;
        int rc = plan_chunk(cfg, coarse, fine, &ios[i], R[i], &p);
        if (rc) return rc;
        plans.push_back(p);
    }
    const int n = (int)plans.size();
    // the final compositing of chunk k-1 runs while chunk k is under way: neighbours need their own workspaces
    for (int i = 0; i + 1 < n; ++i)
        if (plans[i].io->workspace == plans[i + 1].io->workspace)
            return fail(NERF_AMD_EINVAL, "consecutive chunks must use distinct workspaces");
    return walk_chunks(plans.data(), n, stage_field, s);
}

}  // extern "C"

// ---- occupancy grid (occupancy.hip): the grid's entry points, the field at a point list, render_rays over live points ----
namespace {
constexpr double OCC_SAMPLE_REACH = 4096.0;      // nerf_amd_occupancy_sample_points: max(|lo|, |hi|) n / (hi - lo) it vouches for

// the caller's grid, checked, as the kernels take it
int occ_grid(const nerf_amd_occupancy_grid *g, bool need_words, OccGrid *out) {
    if (!g) return fail(NERF_AMD_EINVAL, "null occupancy grid");
    if (need_words && !g->words) return fail(NERF_AMD_EINVAL, "occupancy grid has no words");
    if (g->outside != NERF_AMD_OCC_OUTSIDE_LIVE && g->outside != NERF_AMD_OCC_OUTSIDE_EMPTY)
        return fail(NERF_AMD_EINVAL, "occupancy grid: unknown outside policy");
    out->words = g->words;
    out->outside_live = g->outside == NERF_AMD_OCC_OUTSIDE_LIVE;
    for (int a = 0; a < 3; ++a) {
        if (g->n[a] < 1 || g->n[a] > 1024) return fail(NERF_AMD_EINVAL, "occupancy grid: resolution must be 1..1024 per axis");
        const double lo = g->lo[a], hi = g->hi[a];
        if (!std::isfinite(lo) || !std::isfinite(hi) || !(hi > lo)) return fail(NERF_AMD_EINVAL, "occupancy grid: box must be finite with lo < hi");
        out->lo[a] = g->lo[a];
        out->n[a] = g->n[a];
        out->scale[a] = (float)((double)g->n[a] / (hi - lo));
        out->width[a] = (float)((hi - lo) / (double)g->n[a]);
        out->centre[a] = (float)((lo + hi) / 2.0);
        if (!std::isfinite(out->scale[a]) || !(out->width[a] > 0.0f)) return fail(NERF_AMD_EINVAL, "occupancy grid: box too thin or too wide for fp32");
    }
    return NERF_AMD_OK;
}

int64_t occ_cells(const int32_t n[3]) { return (int64_t)n[0] * n[1] * n[2]; }

// the field at a point list, with the render path's choice of weight stream (stage_field)
int field_points(const nerf_amd_model *m, const float *pts, const float *viewdirs, int64_t n, float *raw, int precision, hipStream_t s) {
    if (n == 0) return NERF_AMD_OK;
    MlpArgs a{};
    set_inputs(a, pts, viewdirs, nullptr, 0, nullptr, true);      // (run_field drops viewdirs for a model without view branch)
    a.P = n; a.S = 1; a.out = raw;
    return run_field(m, a, precision, s, fold_wanted());
}

// scratch of the culled passes behind the dense workspace: one pass's worth, reused by the second
struct CullWs {
    int32_t *rank, *block_counts;
    float *pts, *vd, *raw_live;
    int64_t *count;
};
size_t cull_ws_bytes(int64_t P, int och, CullWs *w, char *base) {
    size_t b = 0;
    auto take = [&](size_t bytes) { char *q = base ? base + b : nullptr; b += align_up(bytes); return q; };
    char *rank = take(P * sizeof(int32_t)), *bc = take(((P + 255) / 256) * sizeof(int32_t)), *pts = take(P * 3 * sizeof(float));
    char *vd = take(P * 3 * sizeof(float)), *rl = take(P * (size_t)och * sizeof(float)), *cnt = take(sizeof(int64_t));
    if (w) {
        w->rank = reinterpret_cast<int32_t *>(rank); w->block_counts = reinterpret_cast<int32_t *>(bc);
        w->pts = reinterpret_cast<float *>(pts); w->vd = reinterpret_cast<float *>(vd); w->raw_live = reinterpret_cast<float *>(rl);
        w->count = reinterpret_cast<int64_t *>(cnt);
    }
    return b;
}

// 8 bytes of pinned host memory per host thread for the live count (portable: any device may write it); kept for the
// life of the process
int64_t *pinned_count() {
    thread_local int64_t *p = nullptr;
    if (!p && hipHostMalloc(reinterpret_cast<void **>(&p), sizeof(int64_t), hipHostMallocPortable) != hipSuccess) p = nullptr;
    return p;
}

// stage_field over the live points of the pass: cull -> count to the host -> field on the compact list -> expand
int stage_field_culled(const ChunkPlan &p, bool fine_pass, const OccGrid &g, const CullWs &w, int64_t *n_live, hipStream_t s) {
    const int S = fine_pass ? p.Nf : p.Nc;
    const float *z = fine_pass ? p.z_f : p.z_c;
    float *raw = fine_pass ? p.raw_f : p.raw_c;
    const nerf_amd_model *m = fine_pass ? p.fm : p.coarse;
    int rc = launch_occupancy_cull(g, p.io->rays, p.io->ray_ch, z, p.R, S, w.block_counts, w.rank, w.pts, p.has_vd ? w.vd : nullptr,
                                   w.count, s);
    if (rc) return fail(rc, "occupancy cull launch failed");
    int64_t *host = pinned_count();
    if (!host) return fail(NERF_AMD_ENOMEM, "no pinned host memory for the live count");
    HIP_TRY(hipMemcpyAsync(host, w.count, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *n_live = *host;
    if (*n_live < 0 || *n_live > p.R * (int64_t)S) return fail(NERF_AMD_EHIP, "occupancy cull returned an impossible count");
    if ((rc = field_points(m, w.pts, p.has_vd ? w.vd : nullptr, *n_live, w.raw_live, p.cfg->precision, s))) return rc;
    rc = launch_occupancy_expand(w.raw_live, w.rank, p.R * (int64_t)S, p.och, raw, s);
    return rc ? fail(rc, "occupancy expand launch failed") : NERF_AMD_OK;
}
}  // namespace

extern "C" {

int nerf_amd_occupancy_query(const nerf_amd_occupancy_grid *grid, const float *pts, int64_t n, uint8_t *live, int32_t *cell,
                             void *stream) {
    OccGrid g;
    if (int rc = occ_grid(grid, true, &g)) return rc;
    if (n < 0 || (n > 0 && (!pts || !live))) return fail(NERF_AMD_EINVAL, "bad occupancy_query arguments");
    int rc = launch_occupancy_query(g, pts, n, live, cell, static_cast<hipStream_t>(stream));
    return rc ? fail(rc, "occupancy_query launch failed") : NERF_AMD_OK;
}

int nerf_amd_occupancy_sample_points(const nerf_amd_occupancy_grid *grid, int64_t c0, int64_t c1, int32_t K, uint32_t seed,
                                     float *pts, void *stream) {
    OccGrid g;
    if (int rc = occ_grid(grid, false, &g)) return rc;
    for (int a = 0; a < 3; ++a) {
        const double lo = grid->lo[a], hi = grid->hi[a];
        if (std::fmax(std::fabs(lo), std::fabs(hi)) * grid->n[a] / (hi - lo) > OCC_SAMPLE_REACH)
            return fail(NERF_AMD_EINVAL, "occupancy_sample_points: the box is too far from the origin for its cell size "
                                         "(max(|lo|, |hi|) n / (hi - lo) must not exceed 4096): samples could leave their cells");
    }
    if (c0 < 0 || c1 < c0 || c1 > occ_cells(grid->n) || K < 1 || (c1 - c0) * (int64_t)K >= ((int64_t)1 << 31) || (c1 > c0 && !pts))
        return fail(NERF_AMD_EINVAL, "bad occupancy_sample_points arguments");
    int rc = launch_occupancy_sample_points(g, c0, c1, K, seed, pts, static_cast<hipStream_t>(stream));
    return rc ? fail(rc, "occupancy_sample_points launch failed") : NERF_AMD_OK;
}

int nerf_amd_occupancy_mark(const float *sigma, int64_t c0, int64_t c1, int32_t K, float threshold, int accumulate,
                            int32_t *words, void *stream) {
    if (c0 < 0 || (c0 & 31) || c1 < c0 || c1 > ((int64_t)1 << 30) || K < 1 || (c1 - c0) * (int64_t)K >= ((int64_t)1 << 31) ||
        (c1 > c0 && (!sigma || !words)))
        return fail(NERF_AMD_EINVAL, "bad occupancy_mark arguments (c0 must be a multiple of 32)");
    int rc = launch_occupancy_mark(sigma, c0, c1, K, threshold, accumulate, words, static_cast<hipStream_t>(stream));
    return rc ? fail(rc, "occupancy_mark launch failed") : NERF_AMD_OK;
}

int nerf_amd_occupancy_dilate(const int32_t *in, int32_t nx, int32_t ny, int32_t nz, int32_t iterations, int32_t *out,
                              void *stream) {
    if (nx < 1 || ny < 1 || nz < 1 || nx > 1024 || ny > 1024 || nz > 1024 || iterations < 0 || !in || !out || in == out)
        return fail(NERF_AMD_EINVAL, "bad occupancy_dilate arguments");
    int rc = launch_occupancy_dilate(in, nx, ny, nz, iterations > 1024 ? 1024 : iterations, out, static_cast<hipStream_t>(stream));
    return rc ? fail(rc, "occupancy_dilate launch failed") : NERF_AMD_OK;
}

int nerf_amd_occupancy_cull(const nerf_amd_occupancy_grid *grid, const float *rays, int32_t ray_ch, const float *z, int64_t R,
                            int32_t S, int32_t *block_counts, int32_t *rank, float *pts_live, float *vd_live, int64_t *count,
                            void *stream) {
    OccGrid g;
    if (int rc = occ_grid(grid, true, &g)) return rc;
    if (R < 0 || S < 1 || (ray_ch != 8 && ray_ch != 11) || R * (int64_t)S >= ((int64_t)1 << 31) || !count ||
        (R > 0 && (!rays || !z || !block_counts || !rank || !pts_live)) || (vd_live && ray_ch != 11))
        return fail(NERF_AMD_EINVAL, "bad occupancy_cull arguments");
    int rc = launch_occupancy_cull(g, rays, ray_ch, z, R, S, block_counts, rank, pts_live, vd_live, count, static_cast<hipStream_t>(stream));
    return rc ? fail(rc, "occupancy_cull launch failed") : NERF_AMD_OK;
}

int nerf_amd_occupancy_expand(const float *raw_live, const int32_t *rank, int64_t n, int32_t ch, float *raw, void *stream) {
    if (n < 0 || ch < 1 || (n > 0 && (!rank || !raw))) return fail(NERF_AMD_EINVAL, "bad occupancy_expand arguments");
    int rc = launch_occupancy_expand(raw_live, rank, n, ch, raw, static_cast<hipStream_t>(stream));
    return rc ? fail(rc, "occupancy_expand launch failed") : NERF_AMD_OK;
}

int nerf_amd_occupancy_cull_capped(const nerf_amd_occupancy_grid *grid, const float *rays, int32_t ray_ch, const float *z, int64_t R,
                                   int32_t S, int64_t capacity, int32_t *block_counts, int32_t *rank, int32_t *src, float *pts_live,
                                   float *vd_live, int64_t *counts, void *stream) {
    OccGrid g;
    if (int rc = occ_grid(grid, true, &g)) return rc;
    if (R < 0 || S < 1 || (ray_ch != 8 && ray_ch != 11) || R * (int64_t)S >= ((int64_t)1 << 31) || capacity < 1 ||
        capacity >= ((int64_t)1 << 31) || !counts || !src || !pts_live || (R > 0 && (!rays || !z || !block_counts || !rank)) ||
        (vd_live && ray_ch != 11))
        return fail(NERF_AMD_EINVAL, "bad occupancy_cull_capped arguments");
    int rc = launch_occupancy_cull_capped(g, rays, ray_ch, z, R, S, capacity, block_counts, rank, src, pts_live, vd_live, counts,
                                          static_cast<hipStream_t>(stream));
    return rc ? fail(rc, "occupancy_cull_capped launch failed") : NERF_AMD_OK;
}

int nerf_amd_occupancy_gather_rows(const float *dense, const int32_t *src, int64_t capacity, int32_t ch, float *live, void *stream) {
    if (capacity < 0 || ch < 1 || (capacity > 0 && (!dense || !src || !live))) return fail(NERF_AMD_EINVAL, "bad occupancy_gather_rows arguments");
    int rc = launch_occupancy_gather_rows(dense, src, capacity, ch, live, static_cast<hipStream_t>(stream));
    return rc ? fail(rc, "occupancy_gather_rows launch failed") : NERF_AMD_OK;
}

int nerf_amd_occupancy_ray_grads(const int32_t *rank, const float *z, const float *g_pts_live, const float *g_vd_live, int64_t R,
                                 int32_t S, int32_t ray_ch, float *g_rays, void *stream) {
    if (R < 0 || S < 1 || (ray_ch != 8 && ray_ch != 11) || R * (int64_t)S >= ((int64_t)1 << 31) ||
        (R > 0 && (!rank || !z || !g_pts_live || !g_rays)) || (g_vd_live && ray_ch != 11))
        return fail(NERF_AMD_EINVAL, "bad occupancy_ray_grads arguments");
    int rc = launch_occupancy_ray_grads(rank, z, g_pts_live, g_vd_live, R, S, ray_ch, g_rays, static_cast<hipStream_t>(stream));
    return rc ? fail(rc, "occupancy_ray_grads launch failed") : NERF_AMD_OK;
}

int nerf_amd_occupancy_ray_bounds(const nerf_amd_occupancy_grid *grid, const float *rays, int32_t ray_ch, int64_t R,
                                  int32_t probes, int32_t pad, float *rays_out, float *bounds, int32_t *span, void *stream) {
    OccGrid g;
    if (int rc = occ_grid(grid, true, &g)) return rc;
    if (R < 0 || R >= ((int64_t)1 << 31) || (ray_ch != 8 && ray_ch != 11) || probes < 64 || probes > 4096 || (probes & (probes - 1)) ||
        pad < 0 || pad > probes || (!rays_out && !bounds && !span) || (R > 0 && !rays) || (rays_out && rays_out == rays))
        return fail(NERF_AMD_EINVAL, "bad occupancy_ray_bounds arguments (probes: a power of two in 64..4096; 0 <= pad <= probes; "
                                     "at least one output; rays_out distinct from rays)");
    int rc = launch_occupancy_ray_bounds(g, rays, ray_ch, R, probes, pad, rays_out, bounds, span, static_cast<hipStream_t>(stream));
    return rc ? fail(rc, "occupancy_ray_bounds launch failed") : NERF_AMD_OK;
}

int nerf_amd_occupancy_coarse_z(const nerf_amd_occupancy_grid *grid, const float *rays, int32_t ray_ch, const float *t_vals,
                                const float *t_rand, int64_t R, int32_t N_samples, int32_t probes, int32_t pad, int lindisp, int perturb,
                                float *z_vals, int32_t *live_count, void *stream) {
    OccGrid g;
    if (int rc = occ_grid(grid, true, &g)) return rc;
    if (lindisp) return fail(NERF_AMD_EINVAL, "occupancy_coarse_z: lindisp is not supported (a warp in disparity is a different definition)");
    if (R < 0 || R >= ((int64_t)1 << 31) || N_samples < 1 || (ray_ch != 8 && ray_ch != 11) || probes < 64 || probes > 4096 ||
        (probes & (probes - 1)) || pad < 0 || pad > probes || (R > 0 && (!rays || !t_vals || !z_vals || (perturb && !t_rand))))
        return fail(NERF_AMD_EINVAL, "bad occupancy_coarse_z arguments (probes: a power of two in 64..4096; 0 <= pad <= probes; "
                                     "t_rand is required under perturb)");
    int rc = launch_occupancy_coarse_z(g, rays, ray_ch, t_vals, perturb ? t_rand : nullptr, R, N_samples, probes, pad, perturb ? 1 : 0,
                                       z_vals, live_count, static_cast<hipStream_t>(stream));
    return rc ? fail(rc, "occupancy_coarse_z launch failed") : NERF_AMD_OK;
}

int nerf_amd_field_points(const nerf_amd_model *m, const float *pts, const float *viewdirs, int64_t n, float *raw,
                          int precision, void *stream) {
    if (!m || n < 0) return fail(NERF_AMD_EINVAL, "bad field_points arguments");
    if (n == 0) return NERF_AMD_OK;
    if (!pts || !raw) return fail(NERF_AMD_EINVAL, "null pts/raw");
    return field_points(m, pts, viewdirs, n, raw, precision, static_cast<hipStream_t>(stream));
}

int64_t nerf_amd_render_rays_culled_workspace(const nerf_amd_render_cfg *cfg, int64_t R, int32_t out_ch) {
    const int64_t dense = nerf_amd_render_rays_workspace(cfg, R, out_ch);
    if (dense < 0 || out_ch < 1 || cfg->N_samples < 1 || cfg->N_importance < 0) return -1;
    return dense + (int64_t)cull_ws_bytes(R * ((int64_t)cfg->N_samples + cfg->N_importance), out_ch, nullptr, nullptr);
}

int nerf_amd_render_rays_culled(const nerf_amd_render_cfg *cfg, const nerf_amd_model *coarse, const nerf_amd_model *fine,
                                const nerf_amd_render_io *io, int64_t R, const nerf_amd_occupancy_grid *grid,
                                int64_t *stats, void *stream) {
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    OccGrid g;
    if (int rc = occ_grid(grid, true, &g)) return rc;
    if (cfg && cfg->use_noise) return fail(NERF_AMD_EINVAL, "render_rays_culled: sigma noise would resurrect culled samples (use_noise must be 0)");
    if (R == 0 && cfg && coarse && io) return NERF_AMD_OK;
    ChunkPlan p;
    if (int rc = plan_chunk(cfg, coarse, fine, io, R, &p)) return rc;
    if (R * (int64_t)p.Nf >= ((int64_t)1 << 31)) return fail(NERF_AMD_EINVAL, "render_rays_culled: R * samples must stay below 2^31");
    if (io->workspace_bytes < nerf_amd_render_rays_culled_workspace(cfg, R, p.och)) return fail(NERF_AMD_EINVAL, "workspace too small");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess || st != hipStreamCaptureStatusNone)
        return fail(NERF_AMD_EINVAL, "render_rays_culled synchronises the stream: it cannot be captured in a graph");
    CullWs w;
    cull_ws_bytes(R * (int64_t)p.Nf, p.och, &w, static_cast<char *>(io->workspace) + nerf_amd_render_rays_workspace(cfg, R, p.och));
    auto field = [&](const ChunkPlan &q, bool fine_pass, hipStream_t fs) {      // the culled field stage; fills its pass's two counts
        int64_t live = 0;
        const int frc = stage_field_culled(q, fine_pass, g, w, &live, fs);
        if (!frc && stats) { stats[fine_pass ? 2 : 0] = live; stats[fine_pass ? 3 : 1] = q.R * (int64_t)(fine_pass ? q.Nf : q.Nc); }
        return frc;
    };
    return walk_chunks(&p, 1, field, s);
}

}  // extern "C"

// ---- Renderer.render_batch as ONE call over contiguous whole-batch buffers -------------------------------------
namespace {
constexpr int64_t SUPER_CHUNK_RAYS = 32768;      // rays per launch group (the reference's own default chunk)
constexpr int BATCH_SLOTS = 3;                   // workspaces in rotation: a group is live from its coarse field to its final compositing

// The side stream and a pool of timing-less events per device.  Streams are created once; events are handed out and
// taken back under the mutex (an event can be re-recorded as soon as every wait on it has been ENQUEUED).
struct SideLane {
    hipStream_t stream = nullptr;
    hipStream_t more[2] = {nullptr, nullptr};      // further streams for work that splits more than two ways (lane_streams)
    std::vector<hipEvent_t> free_events;
};
std::mutex g_lane_mu;
SideLane g_lanes[64];

}  // namespace
namespace na {
namespace {
// Streams and events belong to the device that is current when they are created: make `device` current for the
// creation calls and put the caller's device back afterwards.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int device) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != device) {
            err = hipSetDevice(device);
            switched = err == hipSuccess;
        }
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};
}  // namespace

int lane_acquire(int device, int n_events, hipStream_t *side, std::vector<hipEvent_t> *events) {
    if (device < 0 || device >= 64) return fail(NERF_AMD_EINVAL, "device index out of range");
    std::lock_guard<std::mutex> lk(g_lane_mu);
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return hip_fail(guard.err, "hipSetDevice(lane device)");
    SideLane &l = g_lanes[device];
    if (!l.stream) HIP_TRY(hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking));
    *side = l.stream;
    events->clear();
    for (int i = 0; i < n_events; ++i) {
        hipEvent_t e;
        if (!l.free_events.empty()) { e = l.free_events.back(); l.free_events.pop_back(); }
        else if (hipError_t err = hipEventCreateWithFlags(&e, hipEventDisableTiming); err != hipSuccess) {
            for (hipEvent_t got : *events) l.free_events.push_back(got);      // hand back what was already taken
            events->clear();
            return hip_fail(err, "hipEventCreateWithFlags");
        }
        events->push_back(e);
    }
    return NERF_AMD_OK;
}
int lane_streams(int device, int n, hipStream_t *out) {
    if (device < 0 || device >= 64 || n < 1 || n > 3) return fail(NERF_AMD_EINVAL, "lane_streams: device or count out of range");
    std::lock_guard<std::mutex> lk(g_lane_mu);
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return hip_fail(guard.err, "hipSetDevice(lane device)");
    SideLane &l = g_lanes[device];
    if (!l.stream) HIP_TRY(hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking));
    out[0] = l.stream;
    for (int i = 1; i < n; ++i) {
        if (!l.more[i - 1]) HIP_TRY(hipStreamCreateWithFlags(&l.more[i - 1], hipStreamNonBlocking));
        out[i] = l.more[i - 1];
    }
    return NERF_AMD_OK;
}
void lane_release(int device, const std::vector<hipEvent_t> &events) {
    std::lock_guard<std::mutex> lk(g_lane_mu);
    for (hipEvent_t e : events) g_lanes[device].free_events.push_back(e);
}
}  // namespace na
namespace {

// rows [r0, r0 + R) of a whole-batch io, with `ws` as its workspace
nerf_amd_render_io io_rows(const nerf_amd_render_cfg *cfg, const nerf_amd_render_io &io, int64_t r0, int och, void *ws, int64_t ws_bytes) {
    nerf_amd_render_io o = io;
    const int64_t Nc = cfg->N_samples, Ni = cfg->N_importance, Sl = Nc + Ni;
    auto f = [&](const float *p, int64_t row_floats) { return p ? p + r0 * row_floats : nullptr; };
    auto g = [&](float *p, int64_t row_floats) { return p ? p + r0 * row_floats : nullptr; };
    o.rays = f(io.rays, io.ray_ch);
    o.t_rand = f(io.t_rand, Nc); o.noise0 = f(io.noise0, Nc); o.noise1 = f(io.noise1, Sl);
    o.u = f(io.u, Ni); o.z_coarse = f(io.z_coarse, Nc);
    o.rgb_map = g(io.rgb_map, 3); o.disp_map = g(io.disp_map, 1); o.acc_map = g(io.acc_map, 1);
    o.rgb0 = g(io.rgb0, 3); o.disp0 = g(io.disp0, 1); o.acc0 = g(io.acc0, 1); o.z_std = g(io.z_std, 1);
    o.raw = g(io.raw, Sl * och); o.weights = g(io.weights, Sl); o.z_vals = g(io.z_vals, Sl);
    o.workspace = ws; o.workspace_bytes = ws_bytes;
    return o;
}

int64_t n_super_chunks(int64_t N) { return N <= SUPER_CHUNK_RAYS + SUPER_CHUNK_RAYS / 2 ? 1 : (N + SUPER_CHUNK_RAYS - 1) / SUPER_CHUNK_RAYS; }
}  // namespace

extern "C" {

int64_t nerf_amd_render_batch_workspace(const nerf_amd_render_cfg *cfg, int64_t N, int32_t out_ch) {
    if (!cfg || N < 0) return -1;
    const int64_t n = n_super_chunks(N);
    const int64_t per = nerf_amd_render_rays_workspace(cfg, n == 1 ? N : SUPER_CHUNK_RAYS, out_ch);
    return per * (n < BATCH_SLOTS ? n : BATCH_SLOTS);
}

int nerf_amd_render_batch(const nerf_amd_render_cfg *cfg, const nerf_amd_model *coarse, const nerf_amd_model *fine,
                          const nerf_amd_render_io *io, int64_t N, void *stream) {
    if (!cfg || !coarse || !io || N < 0) return fail(NERF_AMD_EINVAL, "null argument");
    if (N == 0) return NERF_AMD_OK;
    const int64_t n = n_super_chunks(N);
    if (n == 1) return nerf_amd_render_rays(cfg, coarse, fine, io, N, stream);
    const int och = coarse->prog.out_ch;
    const int64_t per = nerf_amd_render_rays_workspace(cfg, SUPER_CHUNK_RAYS, och);
    const int slots = (int)(n < BATCH_SLOTS ? n : BATCH_SLOTS);
    if (!io->workspace || io->workspace_bytes < per * slots) return fail(NERF_AMD_EINVAL, "workspace too small (nerf_amd_render_batch_workspace)");
    if (!io->z_coarse && cfg->perturb && !io->t_rand) return fail(NERF_AMD_EINVAL, "perturb set but neither z_coarse nor t_rand given");

    std::vector<nerf_amd_render_io> ios((size_t)n);
    std::vector<ChunkPlan> plans((size_t)n);
    for (int64_t k = 0; k < n; ++k) {
        const int64_t r0 = k * SUPER_CHUNK_RAYS, R = (k + 1 == n) ? N - r0 : SUPER_CHUNK_RAYS;
        ios[k] = io_rows(cfg, *io, r0, och, static_cast<char *>(io->workspace) + (k % slots) * per, per);
        int rc = plan_chunk(cfg, coarse, fine, &ios[k], R, &plans[k]);
        if (rc) return rc;
    }
    hipStream_t main_s = static_cast<hipStream_t>(stream), side = nullptr;
    const int device = coarse->device;
    const bool two_pass = plans[0].Ni > 0;
    std::vector<hipEvent_t> ev;
    int rc = lane_acquire(device, (int)(3 * n + 1), &side, &ev);
    if (rc) return rc;
    hipEvent_t *ec = ev.data(), *em = ev.data() + n, *ef = ev.data() + 2 * n;   // coarse field done / side-stream stage done / fine field done
    hipEvent_t start = ev[3 * n];
    auto H = [&](hipError_t e, const char *what) { if (e != hipSuccess && !rc) rc = hip_fail(e, what); };
    // the side stream starts behind everything the caller has enqueued so far (inputs, packed weights)
    H(hipEventRecord(start, main_s), "hipEventRecord");
    H(hipStreamWaitEvent(side, start, 0), "hipStreamWaitEvent");

    auto coarse_field = [&](int64_t k) {
        if (k >= slots) H(hipStreamWaitEvent(main_s, em[k - slots + (two_pass ? 1 : 0)], 0), "hipStreamWaitEvent");   // its workspace is free again
        if (!rc) rc = stage_z(plans[k], main_s);
        if (!rc) rc = stage_field(plans[k], false, main_s);
        H(hipEventRecord(ec[k], main_s), "hipEventRecord");
    };
    if (two_pass) {
        // main:  C0 C1 F0 C2 F1 C3 F2 ...        side:  M0  M1+Fin0  M2+Fin1 ... Fin(n-1)
        // M = coarse compositing + resampling (needs C), Fin = final compositing (needs F), both per-ray kernels that run
        // beside the next field kernel instead of between two of them.  A/B 44 (round 4): the fine-pass field kernels on a
        // stream of their own -- F(k) needs M(k), not C(k+1), and with both in flight the workgroups of the one fill the CUs
        // the other's last tiles leave free: 0.4 % faster per view (tools/micro/view_ab.py), bit-identical.  Not the default:
        // with two field kernels resident at once a launch's duration -- what the roofline is read from, in bench.py's events
        // and in rocprofv3's kernel stats alike -- no longer says what the kernel does.
        hipStream_t fine_s = main_s;
        hipStream_t lanes2[2];
        if (g_variant == 44 && lane_streams(device, 2, lanes2) == NERF_AMD_OK) {
            fine_s = lanes2[1];
            H(hipStreamWaitEvent(fine_s, start, 0), "hipStreamWaitEvent");
        }
        coarse_field(0);
        for (int64_t k = 0; k < n && !rc; ++k) {
            if (k + 1 < n) coarse_field(k + 1);
            H(hipStreamWaitEvent(side, ec[k], 0), "hipStreamWaitEvent");
            if (k > 0) H(hipStreamWaitEvent(side, ef[k - 1], 0), "hipStreamWaitEvent");
            if (!rc) rc = stage_mid(plans[k], k > 0 ? &plans[k - 1] : nullptr, side);
            H(hipEventRecord(em[k], side), "hipEventRecord");
            H(hipStreamWaitEvent(fine_s, em[k], 0), "hipStreamWaitEvent");
            if (!rc) rc = stage_field(plans[k], true, fine_s);
            H(hipEventRecord(ef[k], fine_s), "hipEventRecord");
        }
        H(hipStreamWaitEvent(side, ef[n - 1], 0), "hipStreamWaitEvent");
        if (!rc) rc = stage_final(plans[n - 1], side);
    } else {
        for (int64_t k = 0; k < n && !rc; ++k) {
            coarse_field(k);
            H(hipStreamWaitEvent(side, ec[k], 0), "hipStreamWaitEvent");
            if (!rc) rc = stage_final(plans[k], side);
            H(hipEventRecord(em[k], side), "hipEventRecord");
        }
    }
    // the caller's stream continues behind the last per-ray kernel
    H(hipEventRecord(start, side), "hipEventRecord");
    H(hipStreamWaitEvent(main_s, start, 0), "hipStreamWaitEvent");
    lane_release(device, ev);
    return rc;
}

}  // extern "C"

extern "C" {

int nerf_amd_set_tuning(int key, int value) {
    if (key == 0 && value >= 0 && value <= 115) { g_variant.store(value, std::memory_order_relaxed); return NERF_AMD_OK; }
    if (key == 1 && value >= 0 && value <= 1) { g_density_route.store(value, std::memory_order_relaxed); return NERF_AMD_OK; }
    if (key == 2 && value >= 0 && value <= 2) { g_fold.store(value, std::memory_order_relaxed); return NERF_AMD_OK; }
    if (key == 3 && value >= 0 && value <= 1) { g_view_skip_off.store(value, std::memory_order_relaxed); return NERF_AMD_OK; }
    return fail(NERF_AMD_EINVAL, "unknown tuning key/value");
}

int nerf_amd_profile_enable(int on) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_on = on != 0;
    return NERF_AMD_OK;
}

int nerf_amd_profile_collect(int64_t launches[3], double total_ms[3], double total_points[3]) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (int c = 0; c < 3; ++c) { launches[c] = 0; total_ms[c] = 0.0; total_points[c] = 0.0; }
    for (const ProfRec &r : g_prof_recs) {
        float ms = 0.f;
        if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            launches[r.cls] += 1; total_ms[r.cls] += ms; total_points[r.cls] += r.points;
        }
        g_prof_free.emplace_back(r.a, r.b);
    }
    g_prof_recs.clear();
    return NERF_AMD_OK;
}

int nerf_amd_get_rays_backward(int32_t H, int32_t W, const double *K4, int64_t pix0, int64_t n, const float *g_rays_o,
                               const float *g_rays_d, float *g_c2w, void *stream) {
    if (H < 1 || W < 1 || !K4 || pix0 < 0 || n < 0 || pix0 + n > (int64_t)H * W || !g_c2w)
        return fail(NERF_AMD_EINVAL, "bad get_rays_backward arguments");
    int rc = launch_get_rays_bwd(H, W, K4, pix0, n, g_rays_o, g_rays_d, g_c2w, static_cast<hipStream_t>(stream));
    return rc ? fail(rc, "get_rays backward launch failed") : NERF_AMD_OK;
}

int nerf_amd_assemble_rays(const float *rays_o, const float *rays_d, const float *viewdir_src, int64_t n, float near,
                           float far, float *out, void *stream) {
    if (n < 0 || (n > 0 && (!rays_o || !rays_d || !out))) return fail(NERF_AMD_EINVAL, "bad assemble_rays arguments");
    int rc = na::launch_assemble_rays(rays_o, rays_d, viewdir_src, n, near, far, out, static_cast<hipStream_t>(stream));
    return rc ? fail(rc, "assemble_rays launch failed") : NERF_AMD_OK;
}

int nerf_amd_adam_step(int32_t n, float *const *params, const float *const *grads, float *const *exp_avg,
                       float *const *exp_avg_sq, const int64_t *numel, int64_t step, double lr, double beta1,
                       double beta2, double eps, double weight_decay, void *stream) {
    if (n < 0 || step < 1 || (n > 0 && (!params || !grads || !exp_avg || !exp_avg_sq || !numel)))
        return fail(NERF_AMD_EINVAL, "bad adam arguments");
    for (int i = 0; i < n; ++i) {
        if (numel[i] < 0 || numel[i] > 0x7fffffff) return fail(NERF_AMD_EINVAL, "adam: tensor size out of range");
        if (numel[i] > 0 && (!params[i] || !grads[i] || !exp_avg[i] || !exp_avg_sq[i])) return fail(NERF_AMD_EINVAL, "adam: null tensor pointer");
    }
    const double bc1 = 1.0 - std::pow(beta1, (double)step), bc2 = 1.0 - std::pow(beta2, (double)step);
    int rc = na::launch_adam(n, params, grads, exp_avg, exp_avg_sq, numel, (float)(lr / bc1), beta1, beta2,
                             (float)eps, (float)weight_decay, (float)std::sqrt(bc2), static_cast<hipStream_t>(stream));
    return rc ? fail(rc, "adam launch failed") : NERF_AMD_OK;
}

int nerf_amd_adam_step_device(int32_t n, float *const *params, const float *const *grads, float *const *exp_avg,
                              float *const *exp_avg_sq, const int64_t *numel, int64_t *step_dev, const double *lr_dev, double beta1,
                              double beta2, double eps, double weight_decay, float *scalars_dev, void *stream) {
    if (n < 0 || !step_dev || !lr_dev || !scalars_dev || (n > 0 && (!params || !grads || !exp_avg || !exp_avg_sq || !numel)))
        return fail(NERF_AMD_EINVAL, "bad adam arguments");
    if (n > 64) return fail(NERF_AMD_EINVAL, "adam (device scalars): at most 64 tensors per call (one count advance per call)");
    for (int i = 0; i < n; ++i) {
        if (numel[i] < 0 || numel[i] > 0x7fffffff) return fail(NERF_AMD_EINVAL, "adam: tensor size out of range");
        if (numel[i] > 0 && (!params[i] || !grads[i] || !exp_avg[i] || !exp_avg_sq[i])) return fail(NERF_AMD_EINVAL, "adam: null tensor pointer");
    }
    int rc = na::launch_adam(n, params, grads, exp_avg, exp_avg_sq, numel, 0.0f, beta1, beta2, (float)eps, (float)weight_decay, 1.0f,
                             static_cast<hipStream_t>(stream), step_dev, lr_dev, scalars_dev);
    return rc ? fail(rc, "adam launch failed") : NERF_AMD_OK;
}

int nerf_amd_to8b(const float *x, int64_t n, uint8_t *out, void *stream) {
    if (n < 0 || (n > 0 && (!x || !out))) return fail(NERF_AMD_EINVAL, "bad to8b arguments");
    if ((reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(out) & 3))
        return fail(NERF_AMD_EINVAL, "to8b: x must be 16-byte and out 4-byte aligned");
    int rc = launch_to8b(x, n, out, static_cast<hipStream_t>(stream));
    return rc ? fail(rc, "to8b launch failed") : NERF_AMD_OK;
}

// ---- pose estimation and the loss: se(3), rays at pixels, img2mse, each for B hypotheses per launch ------------------
// Every single-pose entry point is its batch twin at B = 1.  The checks that all of them repeat are written once here;
// `name` is the entry point without its prefix, as the messages spell it.
static bool pose_batch_ok(int32_t B) { return B >= 1 && B <= POSE_BATCH_MAX; }
static bool se3_ok(const float *w, const float *v, const float *theta, const float *x, int32_t x_stride) {
    return w && v && theta && x && (x_stride == 0 || x_stride == 16);
}
static bool rays_ok(int32_t H, int32_t W, const double *K4, const int32_t *pix, int64_t n) {
    return H >= 1 && W >= 1 && K4 && n >= 0 && (n == 0 || pix);
}
static bool mse_ok(const float *x, const float *y, int64_t y_stride, int64_t m) { return m >= 1 && x && y && (y_stride == 0 || y_stride == m); }

static int pose_refusal(const char *name, bool args_ok, int32_t B) {
    if (!args_ok) return fail(NERF_AMD_EINVAL, std::string("bad ") + name + " arguments");
    if (!pose_batch_ok(B)) return fail(NERF_AMD_EINVAL, std::string(name) + ": need 1 <= B <= 1024");
    return NERF_AMD_OK;
}
// The launcher's code as the entry point's: `einval` says what the launcher's one refusal (a reduction of more than one
// block without `partials`, kernels.h) means for this entry point.
static int pose_result(const char *name, int rc, const char *einval = nullptr) {
    if (rc == NERF_AMD_OK) return rc;
    return fail(rc, rc == NERF_AMD_EINVAL && einval ? std::string(name) + ": " + einval : std::string(name) + " launch failed");
}
static const char *const ONE_BLOCK_N = "one block per hypothesis, n <= 16384", *const ONE_BLOCK_M = "one block per hypothesis, m <= 16384";

int nerf_amd_se3_transform_batch(const float *w, const float *v, const float *theta, const float *x, int32_t x_stride, int32_t B,
                                 float *T, void *stream) {
    if (int rc = pose_refusal("se3_transform_batch", se3_ok(w, v, theta, x, x_stride) && T, B)) return rc;
    return pose_result("se3_transform_batch", launch_se3_transform(w, v, theta, x, x_stride, B, T, static_cast<hipStream_t>(stream)));
}

int nerf_amd_se3_transform(const float *w, const float *v, const float *theta, const float *x, float *T, void *stream) {
    if (int rc = pose_refusal("se3_transform", se3_ok(w, v, theta, x, 0) && T, 1)) return rc;
    return pose_result("se3_transform", launch_se3_transform(w, v, theta, x, 0, 1, T, static_cast<hipStream_t>(stream)));
}

int nerf_amd_se3_transform_batch_backward(const float *w, const float *v, const float *theta, const float *x, int32_t x_stride,
                                          int32_t B, const float *g_T, float *g_w, float *g_v, float *g_theta, void *stream) {
    if (int rc = pose_refusal("se3_transform_batch_backward", se3_ok(w, v, theta, x, x_stride) && g_T && g_w && g_v && g_theta, B)) return rc;
    return pose_result("se3_transform_batch_backward",
                       launch_se3_transform_bwd(w, v, theta, x, x_stride, B, g_T, g_w, g_v, g_theta, static_cast<hipStream_t>(stream)));
}

int nerf_amd_se3_transform_backward(const float *w, const float *v, const float *theta, const float *x, const float *g_T, float *g_w,
                                    float *g_v, float *g_theta, void *stream) {
    if (int rc = pose_refusal("se3_transform_backward", se3_ok(w, v, theta, x, 0) && g_T && g_w && g_v && g_theta, 1)) return rc;
    return pose_result("se3_transform_backward",
                       launch_se3_transform_bwd(w, v, theta, x, 0, 1, g_T, g_w, g_v, g_theta, static_cast<hipStream_t>(stream)));
}

int nerf_amd_rays_at_pixels_batch(int32_t H, int32_t W, const double *K4, const float *c2w, int64_t c2w_pose_stride,
                                  int32_t c2w_row_stride, int32_t B, const int32_t *pix, int64_t n, float *rays_o, float *rays_d,
                                  void *stream) {
    const bool ok = rays_ok(H, W, K4, pix, n) && c2w && c2w_pose_stride >= 0 && c2w_row_stride >= 4 && (n == 0 || (rays_o && rays_d));
    if (int rc = pose_refusal("rays_at_pixels_batch", ok, B)) return rc;
    return pose_result("rays_at_pixels_batch", launch_rays_at_pixels(K4, c2w, c2w_pose_stride, c2w_row_stride, B, pix, n, rays_o, rays_d,
                                                                     static_cast<hipStream_t>(stream)));
}

int nerf_amd_rays_at_pixels(int32_t H, int32_t W, const double *K4, const float *c2w, int32_t c2w_row_stride, const int32_t *pix,
                            int64_t n, float *rays_o, float *rays_d, void *stream) {
    const bool ok = rays_ok(H, W, K4, pix, n) && c2w && c2w_row_stride >= 4 && (n == 0 || (rays_o && rays_d));
    if (int rc = pose_refusal("rays_at_pixels", ok, 1)) return rc;
    return pose_result("rays_at_pixels",
                       launch_rays_at_pixels(K4, c2w, 0, c2w_row_stride, 1, pix, n, rays_o, rays_d, static_cast<hipStream_t>(stream)));
}

int nerf_amd_rays_at_pixels_batch_backward(int32_t H, int32_t W, const double *K4, const int32_t *pix, int64_t n, int32_t B,
                                           const float *g_rays_o, const float *g_rays_d, float *g_c2w, void *stream) {
    if (int rc = pose_refusal("rays_at_pixels_batch_backward", rays_ok(H, W, K4, pix, n) && g_c2w, B)) return rc;
    return pose_result("rays_at_pixels_batch_backward",
                       launch_rays_at_pixels_bwd(K4, pix, n, B, g_rays_o, g_rays_d, g_c2w, nullptr, static_cast<hipStream_t>(stream)),
                       ONE_BLOCK_N);
}

int nerf_amd_rays_at_pixels_backward(int32_t H, int32_t W, const double *K4, const int32_t *pix, int64_t n, const float *g_rays_o,
                                     const float *g_rays_d, float *g_c2w, float *partials, void *stream) {
    if (int rc = pose_refusal("rays_at_pixels_backward", rays_ok(H, W, K4, pix, n) && g_c2w, 1)) return rc;
    return pose_result("rays_at_pixels_backward",
                       launch_rays_at_pixels_bwd(K4, pix, n, 1, g_rays_o, g_rays_d, g_c2w, partials, static_cast<hipStream_t>(stream)),
                       "n > 16384 needs the partials buffer (256 * 12 floats)");
}

int nerf_amd_rays_at_pixels_indexed(int32_t H, int32_t W, const double *K4, const float *c2w, int64_t c2w_pose_stride,
                                    int32_t c2w_row_stride, int32_t M, const int32_t *pix, const int32_t *pose_index, int64_t n,
                                    float *rays_o, float *rays_d, void *stream) {
    const bool ok = rays_ok(H, W, K4, pix, n) && n <= RAYS_INDEXED_MAX && c2w && c2w_pose_stride >= 0 && c2w_row_stride >= 4 &&
                    (n == 0 || (rays_o && rays_d));
    if (int rc = pose_refusal("rays_at_pixels_indexed", ok, M)) return rc;
    return pose_result("rays_at_pixels_indexed", launch_rays_at_pixels_indexed(H, K4, c2w, c2w_pose_stride, c2w_row_stride, M, pix,
                                                                               pose_index, n, rays_o, rays_d,
                                                                               static_cast<hipStream_t>(stream)));
}

int nerf_amd_rays_at_pixels_indexed_backward(int32_t H, int32_t W, const double *K4, const int32_t *pix, const int32_t *pose_index,
                                             int64_t n, int32_t M, const float *g_rays_o, const float *g_rays_d, float *g_c2w,
                                             void *stream) {
    if (int rc = pose_refusal("rays_at_pixels_indexed_backward", rays_ok(H, W, K4, pix, n) && n <= RAYS_INDEXED_MAX && g_c2w, M)) return rc;
    return pose_result("rays_at_pixels_indexed_backward",
                       launch_rays_at_pixels_indexed_bwd(H, K4, pix, pose_index, n, M, g_rays_o, g_rays_d, g_c2w,
                                                         static_cast<hipStream_t>(stream)));
}

int nerf_amd_se3_exp_batch(const float *xi, const float *x, int32_t x_stride, int32_t M, float *T, void *stream) {
    if (int rc = pose_refusal("se3_exp_batch", xi && x && (x_stride == 0 || x_stride == 16) && T, M)) return rc;
    return pose_result("se3_exp_batch", launch_se3_exp(xi, x, x_stride, M, T, static_cast<hipStream_t>(stream)));
}

int nerf_amd_se3_exp_batch_backward(const float *xi, const float *x, int32_t x_stride, int32_t M, const float *g_T, float *g_xi,
                                    void *stream) {
    if (int rc = pose_refusal("se3_exp_batch_backward", xi && x && (x_stride == 0 || x_stride == 16) && g_T && g_xi, M)) return rc;
    return pose_result("se3_exp_batch_backward", launch_se3_exp_bwd(xi, x, x_stride, M, g_T, g_xi, static_cast<hipStream_t>(stream)));
}

int nerf_amd_img2mse_each(const float *x, const float *y, int64_t y_stride, int64_t m, int32_t B, float *out, void *stream) {
    if (int rc = pose_refusal("img2mse_each", mse_ok(x, y, y_stride, m) && out, B)) return rc;
    return pose_result("img2mse_each", na::launch_img2mse(x, y, y_stride, m, B, out, nullptr, static_cast<hipStream_t>(stream)), ONE_BLOCK_M);
}

int nerf_amd_img2mse(const float *x, const float *y, int64_t n, float *out, float *partials, void *stream) {
    if (int rc = pose_refusal("img2mse", mse_ok(x, y, n, n) && out, 1)) return rc;
    return pose_result("img2mse", na::launch_img2mse(x, y, n, n, 1, out, partials, static_cast<hipStream_t>(stream)),
                       "n > 16384 needs the partials buffer");
}

int nerf_amd_img2mse_each_backward(const float *x, const float *y, int64_t y_stride, int64_t m, int32_t B, const float *g, float *gx,
                                   void *stream) {
    if (int rc = pose_refusal("img2mse_each_backward", mse_ok(x, y, y_stride, m) && g && gx, B)) return rc;
    // no reduction, so nothing in the launcher limits m: the documented limit of the pair is kept here
    if (m > IMG2MSE_EACH_MAX) return fail(NERF_AMD_EINVAL, std::string("img2mse_each_backward: ") + ONE_BLOCK_M);
    return pose_result("img2mse_each_backward",
                       na::launch_img2mse_bwd(x, y, y_stride, m, B, g, gx, nullptr, static_cast<hipStream_t>(stream)));
}

int nerf_amd_img2mse_backward(const float *x, const float *y, int64_t n, const float *g, float *gx, float *gy, void *stream) {
    if (int rc = pose_refusal("img2mse_backward", mse_ok(x, y, n, n) && g, 1)) return rc;
    return pose_result("img2mse_backward", na::launch_img2mse_bwd(x, y, n, n, 1, g, gx, gy, static_cast<hipStream_t>(stream)));
}

int nerf_amd_draw_pixels(int64_t M, int32_t n, uint32_t seed, int64_t *draw_count, const int32_t *region, int32_t H, int32_t W,
                         const float *image, int64_t row_stride, int32_t C, int32_t *pixels, float *target, void *stream) {
    if (H < 1 || W < 1 || C < 3 || row_stride < (int64_t)W * C || !draw_count || !image || !pixels || !target)
        return fail(NERF_AMD_EINVAL, "bad draw_pixels arguments");
    if (M < 1 || M > 0x7fffffff || n < 1 || n > M) return fail(NERF_AMD_EINVAL, "draw_pixels: need 1 <= n <= M <= 2^31 - 1");
    if (!region && M != (int64_t)H * W) return fail(NERF_AMD_EINVAL, "draw_pixels: without a region list M must be H * W");
    int rc = launch_draw_pixels(M, n, seed, draw_count, region, W, image, row_stride, C, pixels, target, static_cast<hipStream_t>(stream));
    return rc ? fail(rc, "draw_pixels launch failed") : NERF_AMD_OK;
}

int64_t nerf_amd_interest_points_workspace(int32_t H, int32_t W) {
    if (H < 1 || W < 1) return 0;
    return 8 + (int64_t)H * W * (8 + 4 + 4);          // the maximum, the int64 responses, gx, gy
}

int nerf_amd_interest_points(const uint8_t *image, int32_t H, int32_t W, int32_t C, int32_t quality, void *workspace, uint8_t *mask,
                             void *stream) {
    if (H < 1 || W < 1 || (int64_t)H * W > 0x7fffffff || (C != 3 && C != 4) || quality < 1 || quality > 100 || !image || !workspace ||
        !mask || (reinterpret_cast<uintptr_t>(workspace) & 7))
        return fail(NERF_AMD_EINVAL, "bad interest_points arguments (C = 3 or 4, quality 1..100, workspace 8-byte aligned)");
    int rc = launch_interest_points(image, H, W, C, quality, workspace, mask, static_cast<hipStream_t>(stream));
    return rc ? fail(rc, "interest_points launch failed") : NERF_AMD_OK;
}

int nerf_amd_dilate_mask(const uint8_t *in, int32_t H, int32_t W, int32_t k, int32_t iterations, uint8_t *out, void *stream) {
    if (H < 1 || W < 1 || (int64_t)H * W > 0x7fffffff || k < 1 || iterations < 1 || (int64_t)k * iterations > 0x7fff || !in || !out ||
        in == out)
        return fail(NERF_AMD_EINVAL, "bad dilate_mask arguments");
    int rc = launch_dilate_mask(in, H, W, k, iterations, out, static_cast<hipStream_t>(stream));
    return rc ? fail(rc, "dilate_mask launch failed") : NERF_AMD_OK;
}

int nerf_amd_compact_mask(const uint8_t *mask, int32_t H, int32_t W, int32_t *block_counts, int32_t *list, int64_t *count, void *stream) {
    if (H < 1 || W < 1 || (int64_t)H * W > 0x7fffffff || !mask || !block_counts || !list || !count)
        return fail(NERF_AMD_EINVAL, "bad compact_mask arguments");
    int rc = launch_compact_mask(mask, H, W, block_counts, list, count, static_cast<hipStream_t>(stream));
    return rc ? fail(rc, "compact_mask launch failed") : NERF_AMD_OK;
}

int nerf_amd_make_rays(int32_t H, int32_t W, const double *K4, const float *c2w, const float *c2w_static,
                       int64_t pix0, int64_t n, float near, float far, int use_viewdirs, int ndc,
                       float *rays_out, void *stream) {
    if (H < 1 || W < 1 || !K4 || !c2w || pix0 < 0 || n < 0 || pix0 + n > (int64_t)H * W || (n > 0 && !rays_out))
        return fail(NERF_AMD_EINVAL, "bad make_rays arguments");
    int rc = launch_make_rays(H, W, K4, c2w, c2w_static, pix0, n, near, far, use_viewdirs, ndc, rays_out,
                              static_cast<hipStream_t>(stream));
    return rc ? fail(rc, "make_rays launch failed") : NERF_AMD_OK;
}

}  // extern "C"
