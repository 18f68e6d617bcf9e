/*
 * nerf_amd.h -- C ABI of the MI355X (gfx950) NeRF volumetric-render hot path.
 *
 * Drop-in boundary for stanford-iprl-lab/nerf_shared's
 *   Renderer.render -> render_batch -> render_rays -> {NeRF.forward/MLP,
 *   raw2outputs, sample_pdf}
 * The reference is pure Python/PyTorch and has no FFI layer of its own
 * (SURVEY.md section 8b), so every entry point below names the Python
 * function (reference file:line) whose arithmetic it replaces; the Python
 * package nerf_shared_amd binds them with ctypes and keeps the reference's
 * class/function signatures.  INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no torch/C++ types.
 *  - Every data pointer is a DEVICE pointer to contiguous fp32 (row-major,
 *    innermost dimension last) unless a parameter says "host".  Buffers are
 *    borrowed: the caller (torch) owns them; the library never frees them.
 *  - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream()
 *    .cuda_stream); all work is enqueued on it, nothing synchronises the host
 *    except nerf_amd_model_create/_update (which read host weights).
 *  - Return value: 0 on success, a negative NERF_AMD_E* code on failure;
 *    nerf_amd_last_error() returns a thread-local message.  No exception
 *    crosses the boundary.
 *  - Re-entrant; the only shared state is inside model handles, which must not
 *    be updated while a launch that uses them is being enqueued.  What the
 *    launchers cache (raised LDS limits, CU counts) is kept per device and
 *    updated atomically (csrc/launch_util.h).
 */
#ifndef NERF_AMD_H
#define NERF_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NERF_AMD_ABI_VERSION 7

#define NERF_AMD_OK            0
#define NERF_AMD_EINVAL       -1   /* bad argument / unsupported shape        */
#define NERF_AMD_EHIP         -2   /* a HIP runtime call failed               */
#define NERF_AMD_EUNSUPPORTED -3   /* architecture not supported by this path */
#define NERF_AMD_ENOMEM       -4

/* Arithmetic of the MLP (the only stage with a precision choice). */
#define NERF_AMD_PREC_FP32 0       /* exact fp32 MFMA (v_mfma_f32_32x32x2_f32): parity mode       */
#define NERF_AMD_PREC_BF16 1       /* bf16 operands, fp32 accumulate (v_mfma_f32_16x16x32_bf16;   */
                                   /* 32x32x16 for output_ch > 16 without a view branch)          */
#define NERF_AMD_PREC_FP32_SPLIT 2 /* fp32-class results on the 16-bit matrix pipe: operands as   */
                                   /* fp16 (hi, lo) pairs, three v_mfma_f32_16x16x32_f16 per      */
                                   /* product, fp32 accumulate (csrc/mlp_split.hip); needs        */
                                   /* |activation| < 65504                                        */

/* Largest R*S of one NERF_AMD_PREC_FP32_SPLIT training call (nerf_amd_field_forward_train / nerf_amd_field_backward),
 * 2^23 - 256: the split weight-gradient kernel addresses its [pad_points(P), <= 256] fp16 planes with 32-bit byte offsets
 * (pad_points(P) * 256 * 2 < 2^32, pad_points(P) = P rounded up to a multiple of 256). */
#define NERF_AMD_SPLIT_TRAIN_MAX_POINTS 8388352

#define NERF_AMD_MAX_SKIPS 8

int         nerf_amd_abi_version(void);
const char *nerf_amd_last_error(void);

/* ------------------------------------------------------------------------
 * Model handle: packed weights of one reference NeRF.
 * Replaces: NeRF.__init__ parameter layout, /root/reference/nerf_shared/nerf.py:62-94.
 * ------------------------------------------------------------------------ */
typedef struct nerf_amd_arch {
    int32_t D;                 /* number of pts_linears                   (nerf.py:62)  */
    int32_t W;                 /* hidden width                                          */
    int32_t output_ch;         /* width of output_linear when !use_viewdirs             */
    int32_t use_viewdirs;
    int32_t multires;          /* L of the xyz encoding (input_ch = 3 + 6 L)            */
    int32_t multires_views;    /* L of the view-direction encoding                      */
    int32_t i_embed;           /* 0 = positional encoding, -1 = identity  (nerf.py:44)  */
    int32_t n_skips;
    int32_t skips[NERF_AMD_MAX_SKIPS];
} nerf_amd_arch;

typedef struct nerf_amd_model nerf_amd_model;   /* opaque, library-owned */

/*
 * Parameters are given in state_dict order as DEVICE pointers to the live fp32
 * nn.Linear tensors ([out,in] row-major weights, [out] biases):
 *   index 0..D-1 : pts_linears.i
 *   viewdirs     : D = feature_linear, D+1 = alpha_linear, D+2 = views_linears.0, D+3 = rgb_linear
 *   no viewdirs  : D = output_linear
 * The library re-packs them on the device (bf16 MFMA A-fragment stream and an
 * fp32 fragment stream) on `stream`; call nerf_amd_model_update again after the
 * parameters change (the Python shim keys this on tensor._version/data_ptr).
 */
int  nerf_amd_model_create(const nerf_amd_arch *arch, int device, nerf_amd_model **out);
int  nerf_amd_model_update(nerf_amd_model *m, const float *const *weights, const float *const *biases,
                           int n_tensors, void *stream);
/*
 * The same for some of the packed copies only (a training step in one precision needs two of the six; re-packing all
 * of them after every optimizer step is 22 us per model of a 1.6-ms step).  `copies`: bit-or of NERF_AMD_COPY_*.
 * `others_current` != 0: the parameters are the ones the OTHER copies were packed from (a copy is being added for the
 * same weights) -- they stay valid; 0: the parameters changed, the other copies become stale.  Every entry point
 * fails with NERF_AMD_EINVAL when the copy it needs is stale or was never packed.  nerf_amd_model_update =
 * NERF_AMD_COPY_ALL.
 */
#define NERF_AMD_COPY_BF16      1   /* bf16 fragment streams + bias tables: NERF_AMD_PREC_BF16 inference and training forward */
#define NERF_AMD_COPY_BWD       2   /* transposed bf16 stream: nerf_amd_field_backward in NERF_AMD_PREC_BF16 */
#define NERF_AMD_COPY_SPLIT     4   /* fp16 (hi, lo) pair stream + bias table: NERF_AMD_PREC_FP32_SPLIT */
#define NERF_AMD_COPY_BWD_SPLIT 8   /* transposed pair stream: nerf_amd_field_backward in split precision */
#define NERF_AMD_COPY_FP32      16  /* fp32 fragment stream + biases: NERF_AMD_PREC_FP32 (inference and training forward), nerf_amd_mlp_embedded */
#define NERF_AMD_COPY_FP32_BWD  32  /* transposed fp32 stream: nerf_amd_field_backward in NERF_AMD_PREC_FP32 */
#define NERF_AMD_COPY_ALL       63
/* The folded bf16 stream of a view-branch model: feature_linear has no activation behind it, so the bf16 render kernels
 * evaluate views_linears.0 on h8 directly through W' = Wv[:, :W] . Wf and b' = Wv[:, :W] . bf + bv, formed in fp32 from the
 * fp32 parameters and rounded to bf16 once (10.9 % fewer MFMAs per point; sigma is bit-identical, rgb moves by less than the
 * mode's own error).  It is NOT part of NERF_AMD_COPY_ALL: it is packed only when this bit is given (two small launches of
 * its own), so a training step packs exactly what it packed before.  nerf_amd_render_batch runs the folded stream when this
 * copy holds the current parameters and the unfolded one otherwise (nerf_amd_set_tuning key 2).  Ignored for models that
 * have nothing to fold (no view branch, or outside the fused family). */
#define NERF_AMD_COPY_BF16_FOLD 128
int  nerf_amd_model_update_copies(nerf_amd_model *m, const float *const *weights, const float *const *biases,
                                  int n_tensors, int copies, int others_current, void *stream);
void nerf_amd_model_destroy(nerf_amd_model *m);
/* 1 when the fused bf16 kernel supports this architecture (D=8, W=256, skips=[4]). */
int  nerf_amd_model_supports_bf16(const nerf_amd_model *m);
/* 1 when the split-precision kernel (NERF_AMD_PREC_FP32_SPLIT) supports this architecture: the same set. */
int  nerf_amd_model_supports_split(const nerf_amd_model *m);
int  nerf_amd_model_out_ch(const nerf_amd_model *m);       /* 4 with viewdirs, else output_ch */

/* Host-side packing of one model into the bf16 fragment stream (test hook: lets
 * CPU tests check the fragment layout without a GPU).  Weights/biases are HOST
 * pointers here.  `stream_out` receives n_frags*512 uint16 (bf16 bits) and
 * `bias_out` the fp32 bias table; pass NULL to query sizes only. */
int  nerf_amd_pack_bf16_host(const nerf_amd_arch *arch, int shape /* 32: 32x32x16 stream, 16: 16x16x32 stream, 17: transposed
                                (backward) stream, 18 / 19: the split-precision forward / transposed streams (fp16 hi, lo fragments),
                                20: the folded 16x16x32 stream of a view-branch model (NERF_AMD_COPY_BF16_FOLD) */,
                             const float *const *weights,
                             const float *const *biases, int n_tensors,
                             uint16_t *stream_out, int64_t *n_frags, float *bias_out, int64_t *n_bias);

/* ------------------------------------------------------------------------
 * a1  Embedder.embed / get_embedder          nerf.py:16-58
 * x [n,3] -> out [n, 3+6*multires]   (frequency-major, sin then cos, xyz innermost)
 * ------------------------------------------------------------------------ */
int nerf_amd_embed(const float *x, int64_t n, int multires, float *out, void *stream);

/* ------------------------------------------------------------------------
 * a3/a4  NeRF.forward + NeRF.MLP              nerf.py:96-134
 * pts [n_rays*n_samples,3]; viewdirs [n_rays,3] (NULL when the model has no
 * view branch; every sample of ray r uses viewdirs[r], nerf.py:101)
 * -> out [n_rays*n_samples, out_ch].  No netchunk: the kernel tiles internally.
 * ------------------------------------------------------------------------ */
int nerf_amd_nerf_forward(const nerf_amd_model *m, const float *pts, const float *viewdirs,
                          int64_t n_rays, int32_t n_samples, float *out, int precision, void *stream);

/* ------------------------------------------------------------------------
 * a4  NeRF.MLP on already-embedded rows       nerf.py:110-134
 * x [n, input_ch + input_ch_views] -> out [n, out_ch]; exact-fp32 kernel.
 * ------------------------------------------------------------------------ */
int nerf_amd_mlp_embedded(const nerf_amd_model *m, const float *x, int64_t n, float *out, void *stream);

/* ------------------------------------------------------------------------
 * a13  utils.ndc_rays on explicit rays        utils.py:54-71
 * rays_o, rays_d [n,3] -> out_o, out_d [n,3]; focal is the Python float K[0][0].
 * ------------------------------------------------------------------------ */
int nerf_amd_ndc_rays(int32_t H, int32_t W, double focal, float near, const float *rays_o, const float *rays_d,
                      int64_t n, float *out_o, float *out_d, void *stream);

/* Backward of nerf_amd_ndc_rays (pose estimation on forward-facing scenes differentiates through the warp):
 * gradients of its two outputs [n,3] (either may be NULL = zero) -> gradients of rays_o / rays_d [n,3]
 * (either may be NULL = not wanted), overwritten. */
int nerf_amd_ndc_rays_backward(int32_t H, int32_t W, double focal, float near, const float *rays_o, const float *rays_d,
                               const float *g_out_o, const float *g_out_d, int64_t n, float *g_rays_o, float *g_rays_d,
                               void *stream);

/* ------------------------------------------------------------------------
 * a10  Renderer.raw2outputs                   render_utils.py:241-290
 * raw [R,S,raw_ch] (channels 0..2 rgb, 3 sigma), z_vals [R,S], rays_d with row
 * stride `rays_d_stride` floats, noise [R,S] or NULL (already scaled by
 * raw_noise_std).  Any output pointer may be NULL.
 * ------------------------------------------------------------------------ */
int nerf_amd_raw2outputs(const float *raw, int32_t raw_ch, const float *z_vals,
                         const float *rays_d, int32_t rays_d_stride, const float *noise,
                         int64_t R, int32_t S, int white_bkgd,
                         float *rgb_map, float *disp_map, float *acc_map, float *weights,
                         float *depth_map, void *stream);

/* Backward of raw2outputs (what autograd derives from render_utils.py:241-290): upstream gradients of
 * the five outputs (any may be NULL) -> g_raw [R,S,raw_ch] and, if asked, g_rays_d [R,3] (the
 * dependence of dists on |rays_d|, :259).  z_vals are constants.  SURVEY.md section 8f-1. */
int nerf_amd_raw2outputs_backward(const float *raw, int32_t raw_ch, const float *z_vals, const float *rays_d,
                                  int32_t rays_d_stride, const float *noise, int64_t R, int32_t S, int white_bkgd,
                                  const float *g_rgb_map, const float *g_disp_map, const float *g_acc_map,
                                  const float *g_depth_map, const float *g_weights, float *g_raw,
                                  float *g_rays_d /* [R,3] or NULL */, void *stream);

/* ------------------------------------------------------------------------
 * Training (what loss.backward() does through NeRF.forward, main.py:85-104).
 * Covered: the D=8, W=256, skips=[4] model with view branch and multires 10/4 or 15/6 (every config the
 * reference ships), or without view branch (the output_linear models of nerf.py:91-94,131-132 -- the default
 * use_viewdirs=False of config_parser.py:50 -- multires 10 or 15, output_ch <= 16: raw / g_raw are [P, output_ch],
 * rays are [R,8], viewdirs NULL); gradients of the parameters,
 * of the points / rays (through the positional encoding) and of the view directions.
 * `precision` (the same value in the three calls of one evaluation):
 *   NERF_AMD_PREC_BF16        bf16 operands / fp32 accumulation (the fast default)
 *   NERF_AMD_PREC_FP32_SPLIT  the reference's arithmetic class: every operand of the forward, of the dX chain and of the
 *                             weight-gradient products an fp16 (hi, lo) pair, three MFMAs per product, fp32 accumulation;
 *                             dL/draw is scaled by a power of two taken from its own maximum (csrc/split.h) and the scale
 *                             comes off exactly at the end.  Gradients agree with fp32 autograd to ~1e-6 relative.
 *                             At most NERF_AMD_SPLIT_TRAIN_MAX_POINTS points per call: a larger R*S returns NERF_AMD_EINVAL
 *                             (checked before the workspace size) -- split such a call into pieces of whole rays.
 *   NERF_AMD_PREC_FP32        exact fp32 (v_mfma_f32_32x32x2_f32 everywhere, csrc/train_f32.hip) for ANY architecture
 *                             nerf_amd_model_create accepts -- what the reference's netdepth / netwidth / skips flags build
 *                             (config_parser.py:18-25); the same gradients (parameters, points / rays, view directions)
 *                             within 1e-6 of fp32 autograd, at the fp32 MFMA rate, and no range limit beyond fp32's (the
 *                             split pairs need |activation| < 65504): the path for models outside the family above and for
 *                             models of the family whose values leave fp16's range.  nerf_amd_model_supports_training(m, precision) says which
 *                             precisions a model trains in.
 *   forward_train : the fused forward (explicit pts + viewdirs, or rays + z_vals with pts = o + d z) that also saves every
 *                   layer's activations in `workspace` (nerf_amd_train_workspace bytes, 256-B aligned)
 *   backward      : dL/draw [P,4] -> gradients of every nn.Linear weight [out,in] and bias [out]
 *                   (fp32 device tensors in nerf_amd_model_update order, overwritten)
 * ------------------------------------------------------------------------ */
int     nerf_amd_model_supports_training(const nerf_amd_model *m, int precision);
int64_t nerf_amd_train_workspace(const nerf_amd_model *m, int64_t n_points, int precision);
int     nerf_amd_field_forward_train(const nerf_amd_model *m, const float *pts /* [R*S,3] or NULL */,
                                     const float *viewdirs /* [R,3], with pts */, const float *rays /* [R,11|8], without pts */,
                                     int32_t ray_ch, const float *z_vals, int64_t R, int32_t S, float *raw,
                                     void *workspace, int64_t workspace_bytes, int precision, void *stream);
int     nerf_amd_field_backward(const nerf_amd_model *m, const float *g_raw /* [R*S,4|output_ch] */,
                                const float *pts, const float *viewdirs, const float *rays, int32_t ray_ch,
                                const float *z_vals, int64_t R, int32_t S /* the forward_train inputs */,
                                void *workspace, int64_t workspace_bytes, float *const *grad_weights,
                                float *const *grad_biases, int n_tensors,
                                float *g_pts /* [R*S,3] overwritten, pts mode, or NULL */,
                                float *g_rays /* [R,6] dL/d(o,d), accumulated (pass zeros), rays mode, or NULL */,
                                float *g_viewdirs /* [R,3] accumulated (pass zeros), or NULL */, int precision, void *stream);
/* The same backward for FROZEN parameters (pose estimation, demo_est_rel_pose.py:87-98; any caller that differentiates
 * the inputs only): the dX chain alone -> g_pts / g_rays / g_viewdirs as above, by the launch nerf_amd_field_backward
 * uses for them (ray gradients accumulate with float atomics in both: equal to rounding, not bit for bit); the
 * weight-gradient products -- the largest launches of a training step -- are not enqueued and no gradient table is
 * taken.  All three precisions. */
int     nerf_amd_field_backward_inputs(const nerf_amd_model *m, const float *g_raw, const float *pts, const float *viewdirs,
                                       const float *rays, int32_t ray_ch, const float *z_vals, int64_t R, int32_t S,
                                       void *workspace, int64_t workspace_bytes, float *g_pts, float *g_rays,
                                       float *g_viewdirs, int precision, void *stream);

/* ------------------------------------------------------------------------
 * a5  NeRF.get_density                        nerf.py:136-143
 * The reference evaluates the whole field with an all-ones view direction and keeps channel 3.  sigma depends on the
 * eight trunk layers and alpha_linear only, so the entry points below take a model WITHOUT view branch: the DENSITY TWIN
 * of a view-branch model (same pts_linears, output_linear = the model's alpha_linear [1, W]: tensor order 0..D-1
 * pts_linears.i, D alpha_linear), or an output_linear model itself, whose LAST channel is sigma.  A model with a view
 * branch is refused with NERF_AMD_EINVAL.  Stale or missing packed copies are refused like everywhere else.
 *
 * nerf_amd_density_arch: arch of the density twin of `in` (same trunk and xyz encoding, no view branch, output_ch 1,
 *   multires_views 0); NERF_AMD_EINVAL for a null pointer or an arch nerf_amd_model_create would refuse.
 * nerf_amd_density: pts [n,3] -> sigma [n]                             replaces nerf.py:141-143, output[..., -1]
 *   on the inference kernel of `precision` (its own store when out_ch == 1; with more channels the rows go to
 *   stream-ordered scratch -- hipMallocAsync on `stream` -- and the last column is copied out).
 * nerf_amd_density_value_grad: pts [n,3] -> sigma [n] and grad [n,3] = d sigma_i / d pts_i (the gradient of sigma
 *   itself; a caller's f'(sigma) is one fp32 multiply afterwards).  Replaces autograd.grad(get_density(p).sum(), p)
 *   on the reference, for frozen parameters.  Two routes, same results class:
 *     fused    (nerf_amd_density_grad_fused == 1): one launch, no workspace (csrc/density_grad.hip) -- NERF_AMD_PREC_BF16,
 *              D=8, W=256, skips=[4], multires 10, output_ch <= 16; needs NERF_AMD_COPY_BF16 | NERF_AMD_COPY_BWD;
 *              bit-equal to the two-launch route (same fragments, same rounding points, no atomics);
 *     two launches: nerf_amd_field_forward_train + nerf_amd_field_backward_inputs with dL/draw = 1 in the sigma
 *              column, in `workspace` (nerf_amd_density_grad_workspace bytes, 256-B aligned) -- every model and
 *              precision nerf_amd_model_supports_training covers, with the packed copies those two calls need.
 *   The fused kernel runs wherever it covers the model (it is the faster route there);
 *   nerf_amd_set_tuning(1, 1) sends every call through the two launches (A/B runs, tests).  n = 0 returns NERF_AMD_OK and
 *   touches nothing.
 * ------------------------------------------------------------------------ */
/* arch of the density twin of `in`: same trunk, no view branch, output_ch 1 */
int     nerf_amd_density_arch(const nerf_amd_arch *in, nerf_amd_arch *out);
/* m: a model WITHOUT view branch (a density twin, or an output_linear model: sigma = last channel) */
int     nerf_amd_density(const nerf_amd_model *m, const float *pts, int64_t n, float *sigma /* [n] */,
                         int precision, void *stream);
int     nerf_amd_density_grad_fused(const nerf_amd_model *m, int precision);       /* 1: one launch, no workspace */
int64_t nerf_amd_density_grad_workspace(const nerf_amd_model *m, int64_t n, int precision);   /* 0 when fused */
int     nerf_amd_density_value_grad(const nerf_amd_model *m, const float *pts, int64_t n, float *sigma /* [n] */,
                                    float *grad /* [n,3] */, void *workspace, int64_t workspace_bytes,
                                    int precision, void *stream);

/* ------------------------------------------------------------------------
 * a11  utils.sample_pdf                       utils.py:74-117
 * bins [R,n_bins], weights [R,n_bins-1], u [R,n_samples] or NULL (then
 * u = t_lin[n_samples], the caller's torch.linspace(0,1,n_samples), det=True).
 * -> samples [R,n_samples]
 * ------------------------------------------------------------------------ */
int nerf_amd_sample_pdf(const float *bins, const float *weights, const float *u, const float *t_lin,
                        int64_t R, int32_t n_bins, int32_t n_samples, float *samples, void *stream);

/* ------------------------------------------------------------------------
 * a9  Renderer.render_rays                    render_utils.py:67-174
 * One call enqueues the whole two-pass pipeline for R rays:
 *   z_vals (lin / lindisp, optional stratified jitter) -> coarse field ->
 *   composite -> sample_pdf -> sort(cat) -> fine field -> composite.
 * ------------------------------------------------------------------------ */
/* The two per-ray stages of render_rays that have no Python-level counterpart of their own, exported
 * for the training path (which runs render_rays stage by stage so autograd can cut in):
 *   coarse_z : z_vals of the coarse pass, lin / lindisp + stratified jitter   render_utils.py:105-129
 *   resample : z_mid -> sample_pdf(weights[1:-1]) -> z_std -> sort(cat)       render_utils.py:140-148,168 */
int nerf_amd_coarse_z(const float *rays, int32_t ray_ch, const float *t_vals, const float *t_rand, int64_t R,
                      int32_t N_samples, int lindisp, int perturb, float *z_vals, void *stream);
int nerf_amd_resample(const float *z_coarse, const float *weights, const float *u, const float *t_lin, int64_t R,
                      int32_t N_samples, int32_t N_importance, float *z_fine, float *z_std, void *stream);

typedef struct nerf_amd_render_cfg {
    int32_t N_samples;
    int32_t N_importance;
    int32_t perturb;           /* perturb > 0                               (:115) */
    int32_t lindisp;
    int32_t white_bkgd;
    int32_t use_noise;         /* raw_noise_std > 0: noise0/noise1 are read (:262) */
    int32_t precision;         /* NERF_AMD_PREC_*                                  */
    int32_t reserved;
} nerf_amd_render_cfg;

typedef struct nerf_amd_render_io {
    /* inputs */
    const float *rays;         /* [R, ray_ch]: o(3) d(3) near far [viewdirs(3)]  (:98-103) */
    int32_t      ray_ch;       /* 8 or 11                                                  */
    int32_t      pad0;
    const float *t_vals;       /* [N_samples]  torch.linspace(0,1,N_samples)      (:105)   */
    const float *t_rand;       /* [R,N_samples] jitter draws, NULL unless perturb (:121)   */
    const float *noise0;       /* [R,N_samples] scaled sigma noise, coarse pass   (:264)   */
    const float *noise1;       /* [R,N_samples+N_importance], fine pass                    */
    const float *u;            /* [R,N_importance] sample_pdf draws; NULL => det  (utils.py:83-86) */
    const float *t_lin_imp;    /* [N_importance] torch.linspace(0,1,N_importance), used when u == NULL */
    const float *z_coarse;     /* optional [R,N_samples]: coarse depths already computed by nerf_amd_coarse_z (a caller
                                  that renders many chunks makes them for all rays in one launch); NULL = computed here
                                  from t_vals / t_rand */
    /* outputs (NULL = not wanted) */
    float *rgb_map, *disp_map, *acc_map;      /* [R,3] [R] [R]  from the last pass         */
    float *rgb0, *disp0, *acc0;               /* coarse-pass maps (N_importance > 0)       */
    float *z_std;                             /* [R]  std(z_samples, unbiased=False) (:168) */
    float *raw;                               /* [R,S_last,out_ch] raw of the last pass    */
    float *weights;                           /* [R,S_last]                                */
    float *z_vals;                            /* [R,S_last]                                */
    /* workspace: nerf_amd_render_rays_workspace(cfg, R, out_ch) bytes, 256-B aligned */
    void   *workspace;
    int64_t workspace_bytes;
} nerf_amd_render_io;

int64_t nerf_amd_render_rays_workspace(const nerf_amd_render_cfg *cfg, int64_t R, int32_t out_ch);
int     nerf_amd_render_rays(const nerf_amd_render_cfg *cfg, const nerf_amd_model *coarse,
                             const nerf_amd_model *fine /* NULL: reuse coarse (:150) */,
                             const nerf_amd_render_io *io, int64_t R, void *stream);

/* Renderer.render_batch (render_utils.py:51-65): the chunk loop around render_rays, as one call.
 * ios[i] / R[i] describe chunk i exactly as for nerf_amd_render_rays (own draws, own output rows);
 * consecutive chunks must have distinct workspaces (two buffers used alternately are enough).
 * Results are those of n calls of nerf_amd_render_rays, all on `stream`.  Between the two field kernels
 * of chunk k a single launch does the coarse compositing + resampling of chunk k AND the final compositing
 * of chunk k-1, so a chunk costs three dependent launches instead of four. */
int     nerf_amd_render_chunks(const nerf_amd_render_cfg *cfg, const nerf_amd_model *coarse,
                               const nerf_amd_model *fine, const nerf_amd_render_io *ios, const int64_t *R,
                               int32_t n_chunks, void *stream);

/* Renderer.render_batch (render_utils.py:51-65) over CONTIGUOUS whole-batch buffers: `io` describes all N rays exactly as
 * for nerf_amd_render_rays (rays [N,ray_ch], draws [N,.] -- made per chunk by the caller, in the reference's order, into
 * rows of one buffer each --, outputs [N,.]); z_coarse [N,N_samples] is normally given (one nerf_amd_coarse_z launch).
 * Results are bit-identical to per-chunk nerf_amd_render_rays calls (every kernel is per-ray independent), but the
 * launches are not tied to the caller's chunk size: rays are processed in groups of 32768, the two field kernels of
 * consecutive groups run back to back on `stream`, and the per-ray kernels (coarse compositing + resampling, final
 * compositing) run on a library-owned side stream BESIDE the next field kernel, ordered with events
 *      stream:  C0 C1 F0 C2 F1 C3 F2 ...          side:  M0  M1+Fin0  M2+Fin1 ...  Fin(n-1)
 * The call returns with `stream` ordered behind the last kernel of either stream.  Workspace:
 * nerf_amd_render_batch_workspace(cfg, N, out_ch) bytes (three groups' scratch in rotation), 256-B aligned. */
int64_t nerf_amd_render_batch_workspace(const nerf_amd_render_cfg *cfg, int64_t N, int32_t out_ch);
int     nerf_amd_render_batch(const nerf_amd_render_cfg *cfg, const nerf_amd_model *coarse,
                              const nerf_amd_model *fine, const nerf_amd_render_io *io, int64_t N, void *stream);

/* ------------------------------------------------------------------------
 * a12/a13 + ray-batch assembly of Renderer.render   utils.py:33-71, render_utils.py:200-226
 * Generates rays for flat pixel range [pix0, pix0+n) of an H x W image straight
 * into the [n, 8|11] batch layout (o, d, near, far, viewdirs), NDC-warped when
 * asked.  K = {fx, fy, cx, cy}; c2w is 12 floats (3x4 row-major), both HOST.
 * c2w_static (HOST, may be NULL) reproduces c2w_staticcam (:208-210).
 * ------------------------------------------------------------------------ */
int nerf_amd_make_rays(int32_t H, int32_t W, const double *K4, const float *c2w, const float *c2w_static,
                       int64_t pix0, int64_t n, float near, float far, int use_viewdirs, int ndc,
                       float *rays_out, void *stream);

/* Backward of get_rays with respect to the pose (utils.py:33-42; what the pose-estimation demo
 * differentiates, demo_est_rel_pose.py:87): gradients of rays_o / rays_d [n,3] (either may be NULL) for
 * flat pixels [pix0, pix0+n) -> g_c2w (12 floats, 3x4 row-major, DEVICE, overwritten). */
int nerf_amd_get_rays_backward(int32_t H, int32_t W, const double *K4, int64_t pix0, int64_t n, const float *g_rays_o,
                               const float *g_rays_d, float *g_c2w, void *stream);

/* ------------------------------------------------------------------------
 * Pose estimation (examples/relative_pose_estimation_demo/demo_est_rel_pose.py:74-98): the loop optimises seven numbers
 * behind a camera pose against a few hundred SELECTED pixels.  Everything below reads the pose from DEVICE memory, so
 * the loop body neither synchronises nor copies to the host and can be captured in a HIP graph.
 *
 * get_rays (utils.py:33-42) at n selected pixels: pix [n,2] int32 DEVICE, (x, y) = (column, row) per ray; c2w DEVICE,
 * rows 0..2 of a camera-to-world matrix, row r at c2w + r * c2w_row_stride floats (4 for a contiguous [3,4] or [4,4]).
 * rays_o / rays_d [n,3] receive exactly what nerf_amd_make_rays writes for pixel y * W + x (same operations, same
 * order).  Pixels are not range-checked on the device (they only enter arithmetic, never an address).
 * ------------------------------------------------------------------------ */
int nerf_amd_rays_at_pixels(int32_t H, int32_t W, const double *K4 /* HOST {fx, fy, cx, cy} */, const float *c2w,
                            int32_t c2w_row_stride, const int32_t *pix, int64_t n, float *rays_o, float *rays_d,
                            void *stream);
/* Its backward with respect to the pose: g_rays_o / g_rays_d [n,3] (either may be NULL = zero) -> g_c2w, 12 floats
 * (3x4 row-major, DEVICE, overwritten): g_c2w[k][m] = sum_i g_rays_d[i][k] dir_i[m], g_c2w[k][3] = sum_i g_rays_o[i][k].
 * Order-fixed: per-thread partial sums, a butterfly reduction inside each wave, the wave sums added in index order; no
 * float atomics, so equal inputs give equal bits.  n <= 16384 is one launch; beyond that `partials` (256 * 12 floats,
 * DEVICE) is required and a second tiny launch adds the per-block sums in block order. */
int nerf_amd_rays_at_pixels_backward(int32_t H, int32_t W, const double *K4, const int32_t *pix, int64_t n,
                                     const float *g_rays_o, const float *g_rays_d, float *g_c2w, float *partials,
                                     void *stream);

/* The demo's camera_transf module (demo_est_rel_pose.py:36-66) as one launch each way.  w[3], v[3], theta[1], x[16]
 * (4x4 row-major) and T[16] are DEVICE fp32:   T = exp_i x,  with K = [w]x (the cross-product matrix of w),
 *   exp_i[:3,:3] = I + sin(theta) K + (1 - cos(theta)) K^2
 *   exp_i[:3,3]  = (theta I + (1 - cos(theta)) K + (theta - sin(theta)) K^2) v          exp_i[3,:] = (0, 0, 0, 1)
 * evaluated in fp64 from the fp32 inputs and rounded once (1 - cos(theta) and theta - sin(theta) cancel in fp32).
 * _backward: g_T[16] -> g_w[3], g_v[3], g_theta[1] (overwritten) from the analytic derivatives; x is a constant. */
int nerf_amd_se3_transform(const float *w, const float *v, const float *theta, const float *x, float *T, void *stream);
int nerf_amd_se3_transform_backward(const float *w, const float *v, const float *theta, const float *x, const float *g_T,
                                    float *g_w, float *g_v, float *g_theta, void *stream);

/* Multi-start pose estimation: B pose hypotheses (1 <= B <= 1024, anything else is NERF_AMD_EINVAL) in one launch each.
 * Each single-pose entry point above, and nerf_amd_img2mse(_backward) below, IS its batch form here at B = 1: one kernel
 * and one launcher per operation, hypothesis b = row b of the grid.  So slice b of a batch result equals a call of the
 * single form on slice b bit for bit.  What the single forms have beyond B = 1 of the batch forms: a `partials` buffer
 * (the two reductions may then take more than one block, any n) and nerf_amd_img2mse_backward's gy.  All buffers fp32
 * DEVICE; no synchronisation, no allocation, no float atomics; capturable.
 *
 * se(3): w [B,3], v [B,3], theta [B], T [B,16]; x at x + b * x_stride floats, x_stride = 0 (one x [16] shared by all
 * hypotheses) or 16 (x [B,16]).  One lane per hypothesis, fp64.  _backward: g_T [B,16] -> g_w [B,3], g_v [B,3], g_theta [B]. */
int nerf_amd_se3_transform_batch(const float *w, const float *v, const float *theta, const float *x, int32_t x_stride,
                                 int32_t B, float *T, void *stream);
int nerf_amd_se3_transform_batch_backward(const float *w, const float *v, const float *theta, const float *x, int32_t x_stride,
                                          int32_t B, const float *g_T, float *g_w, float *g_v, float *g_theta, void *stream);
/* nerf_amd_rays_at_pixels for B poses at the SAME n pixels (shared pixels make the hypotheses' losses comparable): pose b
 * at c2w + b * c2w_pose_stride floats (>= 0), its row r a further r * c2w_row_stride floats on; rays_o / rays_d [B,n,3],
 * one thread per (b, pixel).
 * _backward: g_rays_o / g_rays_d [B,n,3] (either may be NULL = zero) -> g_c2w [B,12] (overwritten), ONE 1024-thread block
 * per hypothesis: nerf_amd_rays_at_pixels_backward's one-launch path (loop, butterfly, wave-order sum), so n <= 16384
 * (beyond it NERF_AMD_EINVAL, also at B = 1: this entry point has no partials); n == 0 zeroes g_c2w. */
int nerf_amd_rays_at_pixels_batch(int32_t H, int32_t W, const double *K4 /* HOST */, const float *c2w, int64_t c2w_pose_stride,
                                  int32_t c2w_row_stride, int32_t B, const int32_t *pix, int64_t n, float *rays_o,
                                  float *rays_d, void *stream);
int nerf_amd_rays_at_pixels_batch_backward(int32_t H, int32_t W, const double *K4, const int32_t *pix, int64_t n, int32_t B,
                                           const float *g_rays_o, const float *g_rays_d, float *g_c2w, void *stream);
/* Joint training of the field and the camera poses (BARF / iMAP-style mapping): a training batch mixes images, so every
 * ray has its OWN pose.  nerf_amd_rays_at_pixels at n pixels where ray i takes pose p_i of the M in the table (1 <= M <=
 * 1024; pose m at c2w + m * c2w_pose_stride floats, its row r a further r * c2w_row_stride floats on, as for
 * nerf_amd_rays_at_pixels_batch); rays_o / rays_d [n,3], row i bit-equal to nerf_amd_rays_at_pixels with pose p_i at that
 * pixel (the same device function).  0 <= n <= 2^31 - 1.
 *   pose_index [n] int32 DEVICE:  p_i = pose_index[i], pix[i] = (x, y) in that image.
 *   pose_index NULL:  pix[i] = (x, y) is a pixel of the M images stacked as one [M H, W] image (what nerf_amd_draw_pixels
 *                     over the stacked bank draws): p_i = y / H, the row is y - p_i H.
 * A p_i outside [0, M) never forms an address: that ray's o and d are NaN and it enters no gradient.
 * _backward: g_rays_o / g_rays_d [n,3] (either may be NULL = zero) -> g_c2w [M,12] (overwritten).  ONE 1024-thread block
 * per pose m runs the loop, butterfly and wave-order sum of nerf_amd_rays_at_pixels_backward's one-block path over ALL n
 * rays, block-strided (so the 16384 limit of the batch form does not apply), and adds a ray's terms only when p_i == m --
 * other rays are skipped, not added as zeros.  Order-fixed, no float atomics: equal inputs give equal bits; with every
 * ray on pose m, row m is bit-equal to nerf_amd_rays_at_pixels_batch_backward at B = 1; a pose without rays gets +0.0. */
int nerf_amd_rays_at_pixels_indexed(int32_t H, int32_t W, const double *K4 /* HOST */, const float *c2w, int64_t c2w_pose_stride,
                                    int32_t c2w_row_stride, int32_t M, const int32_t *pix, const int32_t *pose_index,
                                    int64_t n, float *rays_o, float *rays_d, void *stream);
int nerf_amd_rays_at_pixels_indexed_backward(int32_t H, int32_t W, const double *K4, const int32_t *pix,
                                             const int32_t *pose_index, int64_t n, int32_t M, const float *g_rays_o,
                                             const float *g_rays_d, float *g_c2w, void *stream);
/* se(3) twists: T_m = Exp(xi_m) X_m for M poses (1 <= M <= 1024), xi [M,6] = (omega[3], upsilon[3]), th = |omega|,
 * K = [omega]x:
 *   R = I + A K + B K^2     t = (I + B K + C K^2) upsilon     Exp(xi) = [R t; 0 0 0 1]
 *   A = sin th / th         B = (1 - cos th) / th^2           C = (th - sin th) / th^3
 * X at x + m * x_stride floats, x_stride = 0 (one [16] shared) or 16 ([M,16]); T [M,16].  One lane per pose; fp64 from
 * the fp32 inputs, rounded once.  For th^2 < 1e-2 (th < 0.1) A, B, C and their derivatives A'/th, B'/th, C'/th are FIVE
 * Taylor terms in th^2 (through th^8; truncation below 3e-18 relative); above it the closed forms, with 1 - cos th as
 * 2 sin^2(th / 2), lose at most 2 eps64 / th^4 = 2e-10 relative (C'/th; C: 6 eps64 / th^2 < 1e-13) to cancellation, against
 * an fp32 ulp of 6e-8.  xi_m = 0 gives T_m = X_m bit for bit.  Unlike nerf_amd_se3_transform's (w, v, theta), whose pose
 * is bilinear in theta and (w, v) and has no derivative at zero, the twist's derivative at xi = 0 is the six generators
 * applied to X: a correction can START at "none".
 * _backward: g_T [M,16] -> g_xi [M,6] (overwritten), analytic in fp64, at xi = 0 too; X is a constant. */
int nerf_amd_se3_exp_batch(const float *xi, const float *x, int32_t x_stride, int32_t M, float *T, void *stream);
int nerf_amd_se3_exp_batch_backward(const float *xi, const float *x, int32_t x_stride, int32_t M, const float *g_T,
                                    float *g_xi, void *stream);
/* One loss per hypothesis: out[b] = mean((x[b] - y_b)^2), x [B,m]; y_b at y + b * y_stride floats, y_stride = 0 (one y [m]
 * shared) or m (y [B,m]).  One block per hypothesis: nerf_amd_img2mse's one-launch path, so 1 <= m <= 16384
 * (beyond it NERF_AMD_EINVAL, also at B = 1).  _backward: gx[b,i] = g[b] * 2 (x[b,i] - y_b[i]) / m, g [B] DEVICE, gx [B,m]. */
int nerf_amd_img2mse_each(const float *x, const float *y, int64_t y_stride, int64_t m, int32_t B, float *out, void *stream);
int nerf_amd_img2mse_each_backward(const float *x, const float *y, int64_t y_stride, int64_t m, int32_t B, const float *g,
                                   float *gx, void *stream);

/* ------------------------------------------------------------------------
 * Pixel selection for pose estimation (demo_est_rel_pose.py:35-47 and :75-79): where the loop looks.  Integer arithmetic
 * and plain loads / stores only, so every result below is DEFINED exactly (tests compare for equality).  All launches go
 * on `stream` and can be captured; nothing synchronises or allocates.
 *
 * The per-step draw (np.random.choice(M, n, replace=False), interest_regions[rand_inds], obs_img[y, x] in one launch):
 * n distinct indices out of [0, M), their pixels [n,2] int32 (x, y) and their colours target [n,3] fp32.
 *   region NULL:  index i is pixel (i % W, i / W) of the whole image; M must be H * W.
 *   region [M,2] int32 DEVICE (x, y), every entry inside the image (trusted: it addresses the image).
 *   image: fp32 DEVICE, pixel (x, y) at image + y * row_stride + x * C floats, C >= 3 (the first three are gathered).
 * The draw is a keyed bijection of [0, M) evaluated at slots 0..n-1 (distinct by construction, O(1) per thread, no
 * scratch).  All arithmetic uint32 mod 2^32:
 *   mix(x):  x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 *   b = max(1, ceil(bit_length(M - 1) / 2)),  mask = 2^b - 1
 *   k_r = mix(mix(seed + 0x9e3779b9 (r + 1)) ^ draw),  r = 0..3,  draw = the low 32 bits of *draw_count
 *   perm(i): x = i; repeat { L = x >> b; R = x & mask; four times (L, R) = (R, L ^ (mix(R ^ k_r) & mask)); x = (L << b) | R }
 *            until x < M
 * (four Feistel rounds on [0, 4^b), walked along the cycle that starts below M; the domain is under 4 M, so under four
 * rounds on average).  *draw_count (int64, DEVICE) is read by the draw and advanced by one behind it in the stream:
 * replays of a captured call give draws k, k + 1, ... with no host write.  Draws 2^32 apart repeat.
 * 1 <= n <= M <= 2^31 - 1. */
int nerf_amd_draw_pixels(int64_t M, int32_t n, uint32_t seed, int64_t *draw_count, const int32_t *region, int32_t H,
                         int32_t W, const float *image, int64_t row_stride, int32_t C, int32_t *pixels, float *target,
                         void *stream);

/* Interest points of a sensor image: the built-in STAND-IN for the demo's find_POI (cv2 SIFT, demo_est_rel_pose.py:151-164),
 * which is defined here rather than matched: exact integer Harris corners.  image uint8 [H,W,C] DEVICE, C = 3 or 4.
 *   gray = (4899 R + 9617 G + 1868 B + 8192) >> 14;  3x3 Sobel gx, gy at clamped coordinates;
 *   Sxx, Syy, Sxy = sums of gx^2, gy^2, gx gy over the 5x5 window at clamped coordinates;
 *   Rsp = 25 (Sxx Syy - Sxy^2) - (Sxx + Syy)^2 in int64 (k = 0.04; every term below 1.8e16).
 * mask[y,x] (uint8 [H,W] DEVICE) = 1 where Rsp > 0, 100 Rsp >= quality max(Rsp) (quality: integer percent, 1..100), and
 * Rsp is greater than its 3x3 neighbours earlier in row-major order and >= those later (off-image neighbours do not
 * count); 0 elsewhere.  The maximum is an integer atomic max: deterministic.
 * workspace: DEVICE, 8-byte aligned, nerf_amd_interest_points_workspace(H, W) bytes. */
int64_t nerf_amd_interest_points_workspace(int32_t H, int32_t W);
int nerf_amd_interest_points(const uint8_t *image, int32_t H, int32_t W, int32_t C, int32_t quality, void *workspace,
                             uint8_t *mask, void *stream);

/* cv2.dilate(mask, ones((k, k)), iterations=I) by its documented definition (demo_est_rel_pose.py:45): one iteration is
 * out[y,x] = max over dy, dx in [-a, k - 1 - a], a = k / 2, of in[y + dy, x + dx], off-image pixels ignored; the result
 * equals I successive iterations (also for even k, whose window is off-centre).  in / out uint8 [H,W] DEVICE, distinct. */
int nerf_amd_dilate_mask(const uint8_t *in, int32_t H, int32_t W, int32_t k, int32_t iterations, uint8_t *out, void *stream);

/* coords[mask] (demo_est_rel_pose.py:39-47): the (x, y) of the non-zero pixels of mask (uint8 [H,W] DEVICE) in row-major
 * order -> list [*count, 2] int32 DEVICE (room for H * W entries), *count int64 DEVICE.  Stable: counts per 256 pixels,
 * a scan, then each pixel written at its rank; no atomics.  block_counts: (H * W + 255) / 256 int32 of DEVICE scratch. */
int nerf_amd_compact_mask(const uint8_t *mask, int32_t H, int32_t W, int32_t *block_counts, int32_t *list, int64_t *count,
                          void *stream);

/* ------------------------------------------------------------------------
 * Occupancy grid: render without evaluating the field in empty space.  OPT-IN: nothing above reads a grid.
 * Plain loads / stores, integer arithmetic and fp32 operations rounded one by one (no contraction), no float atomics and
 * no atomics on the grid (one thread writes each whole 32-bit word), so every result below is DEFINED exactly and tests
 * compare for equality.
 *
 * The grid is an axis-aligned box lo[3] < hi[3] (finite) with resolution n[3], each 1..1024, in the coordinates the field
 * is evaluated in (for NDC-warped rays: NDC coordinates, e.g. a box around [-1, 1]^3).  Cell (ix, iy, iz) has the linear
 * index c = (ix n[1] + iy) n[2] + iz and is bit (c & 31) of int32 word (c >> 5) of `words` (DEVICE,
 * (n[0] n[1] n[2] + 31) / 32 words; the unused bits of the last word are 0).
 * Lookup of a point p, per axis a, in fp32 with two rounded operations:
 *   t_a = (p_a - lo_a) * scale_a,   scale_a = float32(n_a / (hi_a - lo_a)) formed in double on the host and rounded once,
 *   i_a = floor(t_a);   p is OUTSIDE when on any axis !(t_a >= 0 && t_a < n_a) (this includes NaN), else in cell (i_x, i_y, i_z).
 * An outside point is live under NERF_AMD_OCC_OUTSIDE_LIVE (conservative: the grid only ever removes points it covers) and
 * dead under NERF_AMD_OCC_OUTSIDE_EMPTY (a bounded object, such as the Blender scenes); an inside point is live when its bit is set.
 * Every entry point refuses (NERF_AMD_EINVAL) a grid outside these limits.
 * ------------------------------------------------------------------------ */
#define NERF_AMD_OCC_OUTSIDE_LIVE  0
#define NERF_AMD_OCC_OUTSIDE_EMPTY 1
typedef struct nerf_amd_occupancy_grid {
    const int32_t *words;      /* DEVICE bit words; may be NULL where only the geometry is read (sample_points) */
    float   lo[3], hi[3];
    int32_t n[3];
    int32_t outside;           /* NERF_AMD_OCC_OUTSIDE_* */
} nerf_amd_occupancy_grid;

/* The lookup alone: pts [n,3] fp32 DEVICE -> live [n] uint8 (1 / 0) and, unless NULL, cell [n] int32 (c, or -1 outside). */
int nerf_amd_occupancy_query(const nerf_amd_occupancy_grid *grid, const float *pts, int64_t n, uint8_t *live, int32_t *cell,
                             void *stream);

/* K sample points in each of the cells [c0, c1): pts [(c1 - c0) K, 3], sample j of cell c at row (c - c0) K + j.
 * Per axis a:  p_a = lo_a + (i_a + f_a) * w_a  (two rounded fp32 operations; i_a + f_a is exact),
 *   w_a = float32((hi_a - lo_a) / n_a) formed in double on the host and rounded once,
 *   sample 0 is the cell centre, f = (0.5, 0.5, 0.5);  samples j >= 1 are a keyed-hash jitter on an 8-bit lattice:
 *   h = mix(mix(seed + 0x9e3779b9 j) ^ c)     (uint32 mod 2^32; mix() as defined for nerf_amd_draw_pixels above)
 *   f_x = ((h & 255) + 0.5) / 256,  f_y = (((h >> 8) & 255) + 0.5) / 256,  f_z = (((h >> 16) & 255) + 0.5) / 256,
 * so a sample lies at least 1/512 of a cell from every face of its cell, and it LOOKS UP TO ITS OWN CELL: the rounding
 * errors of forming p and of the lookup add up to less than 2^-11 of a cell wherever
 *   max(|lo_a|, |hi_a|) n_a / (hi_a - lo_a) <= 4096   on every axis
 * (a box within a few thousand cell widths of the origin); a grid beyond that is refused here (NERF_AMD_EINVAL).
 * 0 <= c0 <= c1 <= n[0] n[1] n[2], K >= 1, (c1 - c0) K < 2^31. */
int nerf_amd_occupancy_sample_points(const nerf_amd_occupancy_grid *grid, int64_t c0, int64_t c1, int32_t K, uint32_t seed,
                                     float *pts, void *stream);

/* Sets the bits of the cells [c0, c1) from sigma [(c1 - c0) K] (the density at the rows of sample_points):
 * bit c = any_j(sigma[(c - c0) K + j] > threshold); NaN compares false.  c0 is a multiple of 32, so every word belongs to one
 * thread; the bits of a touched word beyond c1 become 0 (accumulate == 0) or stay (accumulate != 0).  With accumulate != 0
 * the new bits are ORed into the words -- how a second model is added to a grid. */
int nerf_amd_occupancy_mark(const float *sigma, int64_t c0, int64_t c1, int32_t K, float threshold, int accumulate,
                            int32_t *words, void *stream);

/* `iterations` rounds of 3 x 3 x 3 box dilation of the bits of an nx x ny x nz grid, in -> out (DEVICE words, distinct):
 * one round sets a cell when any of its 27 neighbours (itself included) is set, off-grid neighbours ignored.  The rounds
 * compose into one maximum over the (2 iterations + 1)^3 window, which is what is computed; 0 iterations copy.
 * The unused bits of the last word of `out` are 0. */
int nerf_amd_occupancy_dilate(const int32_t *in, int32_t nx, int32_t ny, int32_t nz, int32_t iterations, int32_t *out,
                              void *stream);

/* The per-view kernel: which sample points of rays [R, 8|11] at depths z [R,S] are live.  Point r S + s is
 * rays_o + rays_d z, the product rounded before the sum -- the two operations of the field kernels in their rays + z_vals
 * mode, so the bits are theirs -- looked up as above.  Written stably, in point order:
 *   rank [R S] int32: the position of the point in the compact list, or -1 if culled;
 *   pts_live [*count, 3] (room for R S rows);  vd_live [*count, 3] = the ray's view direction (columns 8..10), when
 *   ray_ch == 11 (else NULL);  *count int64 DEVICE.
 * Three launches -- counts per 256 points, one scan, write at rank -- and no atomics.
 * block_counts: (R S + 255) / 256 int32 of DEVICE scratch.  R S < 2^31. */
int nerf_amd_occupancy_cull(const nerf_amd_occupancy_grid *grid, const float *rays, int32_t ray_ch, const float *z, int64_t R,
                            int32_t S, int32_t *block_counts, int32_t *rank, float *pts_live, float *vd_live, int64_t *count,
                            void *stream);

/* The inverse: raw [n, ch] from raw_live [*, ch] and rank [n]: row i = raw_live[rank[i]], or +0.0 in every channel where
 * rank[i] < 0 (a zero sigma gives alpha 0 and weight 0 in raw2outputs).  One thread per dense row, no memset. */
int nerf_amd_occupancy_expand(const float *raw_live, const int32_t *rank, int64_t n, int32_t ch, float *raw, void *stream);

/* nerf_amd_occupancy_cull into a list of FIXED capacity (training and pose estimation: no count reaches the host, so the
 * caller sizes its field launches by `capacity` and the whole step can be captured in a graph).  1 <= capacity < 2^31,
 * R S < 2^31.  A point is KEPT iff it is live and its stable rank among the live points (point order) is < capacity.
 *   rank [R S] int32: the row of the point in the compact list, or -1 when culled or over the cap;
 *   src [capacity] int32: the dense index r S + s of compact row i, or -1 for a padding row;
 *   pts_live [capacity, 3], vd_live [capacity, 3] (ray_ch == 11, else NULL): kept rows hold the bits
 *     nerf_amd_occupancy_cull writes; the PADDING rows [kept, capacity) hold the point float32((lo_a + hi_a) / 2) per axis
 *     (the box centre, formed in double on the host and rounded once) and the view direction (0, 0, 1) -- a fixed finite
 *     point, so the field is finite there and a zero dL/draw row contributes 0 * finite = 0 to every gradient;
 *   counts int64 DEVICE [2] = {live, kept = min(live, capacity)}, overwritten.
 * Count -> scan -> write like nerf_amd_occupancy_cull; the write launch covers max(R S, capacity) threads, so the padding
 * rows need no host value.  R == 0 writes counts {0, 0} and a list that is all padding (rays, z, rank, block_counts may
 * then be NULL).  block_counts: (R S + 255) / 256 int32 of DEVICE scratch. */
int nerf_amd_occupancy_cull_capped(const nerf_amd_occupancy_grid *grid, const float *rays, int32_t ray_ch, const float *z, int64_t R,
                                   int32_t S, int64_t capacity, int32_t *block_counts, int32_t *rank, int32_t *src, float *pts_live,
                                   float *vd_live, int64_t *counts, void *stream);

/* The backward of nerf_amd_occupancy_expand: dense [n, ch], src [capacity] -> live [capacity, ch]: row i = dense[src[i]], or
 * +0.0 in every channel where src[i] < 0.  One thread per compact row. */
int nerf_amd_occupancy_gather_rows(const float *dense, const int32_t *src, int64_t capacity, int32_t ch, float *live, void *stream);

/* The backward of "pts = o + d z at the kept samples" (and of "view direction of the kept samples") onto the ray batch:
 * rank [R S] and z [R, S] as above, g_pts_live [capacity, 3], g_vd_live [capacity, 3] or NULL -> g_rays [R, ray_ch],
 * overwritten.  Per ray, summed over its KEPT samples (rank >= 0) only:
 *   columns 0..2 = sum_s g_pts;   columns 3..5 = sum_s (g_pts * z), each product rounded before it is added;
 *   columns 6, 7 = 0;   columns 8..10 (ray_ch == 11) = sum_s g_vd (0 when g_vd_live is NULL).
 * Summation order, per column, in fp32: 64 partial sums start at +0.0; partial l adds the terms of the kept samples
 * s = l, l + 64, l + 128, ... in ascending order; then for m = 32, 16, 8, 4, 2, 1 in turn every partial becomes
 * v_l = v_l + v_(l xor m) (all 64 at once), and the result is partial 0.  One 64-lane wave per ray, no atomics. */
int nerf_amd_occupancy_ray_grads(const int32_t *rank, const float *z, const float *g_pts_live, const float *g_vd_live, int64_t R,
                                 int32_t S, int32_t ray_ch, float *g_rays, void *stream);

/* Ray bounds: each ray's near / far (columns 6, 7 of rays [R, 8|11]) clipped to the span over which the grid is live
 * along it, so that a sampler that reads near / far per ray puts its samples where the scene is.  probes = P is a power
 * of two in 64..4096, 0 <= pad <= P, R < 2^31.  Per ray, with near = rays[r,6], far = rays[r,7], in fp32 operations
 * rounded one by one:
 *   w = far - near;   probe k (0 <= k < P) sits at t_k = near + w * u_k, u_k = (k + 0.5) / P (exact), the product
 *   rounded, then the sum;  its point is rays_o + rays_d t_k, the product rounded first (the two operations of
 *   nerf_amd_occupancy_cull);  it is LIVE by the lookup and the outside policy above (a NaN point is outside).
 *   first = the smallest, last = the largest live k.
 *   No live probe (a MISS):  span = (-1, -1), (near', far') = (near, far), the input bits.
 *   Otherwise span = (first, last), k0 = max(first - pad, 0), k1 = min(last + pad, P - 1),
 *     near' = near (the input bits) when k0 == 0,     else near + w * (k0 / P),
 *     far'  = far  (the input bits) when k1 == P - 1, else near + w * ((k1 + 1) / P)      (k / P is exact).
 * Outputs, each optional (NULL) but at least one given:  rays_out [R, ray_ch], distinct from rays: row r of rays with
 * columns 6, 7 replaced by near', far', every other column copied;  bounds [R, 2] = (near', far');  span [R, 2] int32.
 * R == 0 returns NERF_AMD_OK and launches nothing.  One 64-lane wave per ray, 64 probes a round, the round's live mask
 * by ballot; no atomics, enqueue-only (it can be captured; the grid's words are read when it runs).
 * PROMISED:  near <= near' <= far' <= far whenever near <= far and far - near are finite.  The result does not depend
 *   on how many rounds the kernel skips.  For a CONVEX live set and pad >= 1 no point of [near, far] that looks up live
 *   is left out, up to the rounding of the lookup: the live stretch is one interval, it is either shorter than a probe
 *   spacing w / P (see below) or its ends lie within one spacing of first and last, which pad >= 1 covers.
 * NOT PROMISED:  a live stretch shorter than one probe spacing w / P that lies beyond the outermost probed-live stretch
 *   (or is the only one: the ray then counts as a miss) can be left out.  Gaps between first and last are kept: the
 *   culls remove them.  Clipping is NOT idempotent: a second clip probes the narrowed interval and narrows it again. */
int nerf_amd_occupancy_ray_bounds(const nerf_amd_occupancy_grid *grid, const float *rays, int32_t ray_ch, int64_t R,
                                  int32_t probes, int32_t pad, float *rays_out, float *bounds, int32_t *span, void *stream);

/* Coarse depths in each ray's live stretches: the reference's stratified ladder in t in [0, 1] is kept, draw for draw, and
 * mapped through the ray's live probes, so that equal steps of t are equal steps of LIVE length and no coarse sample is spent
 * on the empty stretches inside (or outside) the ray's live span.  rays [R, 8|11], probes = P a power of two in 64..4096,
 * 0 <= pad <= P, R < 2^31, t_vals [N_samples] in [0, 1] ascending (the reference's linspace), t_rand [R, N_samples] in [0, 1)
 * required iff perturb; z_vals [R, N_samples]; live_count int32 [R], optional (NULL), receives L.  All arithmetic is fp32,
 * every operation rounded on its own.  Per ray, with near = rays[r,6], far = rays[r,7]:
 *   1. PROBES, exactly those of nerf_amd_occupancy_ray_bounds:  w = far - near;  probe k (0 <= k < P) sits at
 *      t_k = near + w * ((k + 0.5) / P), the product rounded, then the sum;  its point is rays_o + rays_d t_k, the product
 *      rounded first;  b_k = 1 when it is live by the lookup and the outside policy above (a NaN point is outside).
 *   2. PAD:  b'_k = OR of b_j over |j - k| <= pad, 0 <= j < P.  L = the number of set b';  l_0 < ... < l_(L-1) their indices.
 *   3. FALLBACK:  if L == 0 (a miss) or L == P (all live) the row is nerf_amd_coarse_z's for that ray, bit for bit,
 *      its jitter in z under perturb included (one function, csrc/coarse_ladder.h, serves both kernels) -- so an
 *      all-live grid gives what no sampler gives.
 *   4. WARP, otherwise, for sample s:  t = t_vals[s] without perturb;  with perturb
 *        lower = s > 0 ? 0.5 * (t_s + t_(s-1)) : t_s;   upper = s < N_samples - 1 ? 0.5 * (t_(s+1) + t_s) : t_s;
 *        t = lower + (upper - lower) * t_rand[r, s];
 *      then   a = min(t * (float)L, (float)L);   j = min((int)floorf(a), L - 1);   f = a - (float)j;
 *             e = (float)l_j + f;   u = e * (1 / P) (exact);   z = near + w * u, the product rounded first.
 *   5. lindisp != 0 is refused (NERF_AMD_EINVAL): a warp in disparity is a different definition.
 * Bad probes, pad, grid, rays or a missing buffer are refused before any launch; R == 0 returns NERF_AMD_OK and launches
 * nothing.  One 64-lane wave per ray; the live string is kept one 64-bit word per lane (no LDS, no atomics, no global
 * scratch); enqueue-only (it can be captured; the grid's words are read when it runs).
 * PROMISED (for t in [0, 1] and finite w >= 0):  rows are non-decreasing in s;  e lies in [l_j, l_j + 1]: every sample lies
 *   in a probe interval [near + w k / P, near + w (k + 1) / P] whose padded bit is set, or exactly on that interval's
 *   upper end;  near <= z <= near (+) (far (-) near), the rounded sum of the rounded difference.
 * NOT PROMISED:  z <= far -- the last sample can exceed far by the rounding of near + (far - near) (seen: 4.8e-7 at far
 *   near 6);  that a sample looks up live -- only the probe midpoints were looked up;  anything about a live stretch
 *   shorter than one probe spacing w / P, which the probes can miss.  The depths span the gaps: compositing takes the
 *   distance from the last sample of a stretch to the first of the next as that sample's interval, and the bins of the
 *   hierarchical resampling can span a gap. */
int nerf_amd_occupancy_coarse_z(const nerf_amd_occupancy_grid *grid, const float *rays, int32_t ray_ch, const float *t_vals,
                                const float *t_rand, int64_t R, int32_t N_samples, int32_t probes, int32_t pad, int lindisp,
                                int perturb, float *z_vals, int32_t *live_count, void *stream);

/* The field at a point list: pts [n,3], viewdirs [n,3] (one per POINT; NULL for a model without view branch) -> raw [n,ch].
 * Unlike nerf_amd_nerf_forward it takes the RENDER path's choice of weight stream (tuning key 2: the folded stream of a
 * bf16 view-branch model when NERF_AMD_COPY_BF16_FOLD is current), so a compacted pass runs the kernel the dense pass
 * runs and live rows are bit-equal to the dense ones.  n == 0 returns NERF_AMD_OK and launches nothing.  n < 2^31. */
int nerf_amd_field_points(const nerf_amd_model *m, const float *pts, const float *viewdirs, int64_t n, float *raw,
                          int precision, void *stream);

/* nerf_amd_render_rays with the field evaluated at live points only: each pass is cull -> live count to the host ->
 * nerf_amd_field_points on the compact list -> expand, and everything else (z_vals, compositing, resampling) is the
 * dense code on a dense raw, so outputs have the usual layout; culled samples have raw = +0.0.
 * SYNCHRONISES: the live count has to size the field launch, so each pass copies 8 bytes into pinned host memory and
 * waits for `stream` (once with N_importance == 0, twice otherwise).  It therefore CANNOT be captured in a graph (a
 * capturing stream is refused) and blocks the calling thread.  A pass with no live point launches no field kernel.
 * cfg->use_noise is refused (NERF_AMD_EINVAL): sigma noise would resurrect culled samples.
 * io->workspace: nerf_amd_render_rays_culled_workspace(cfg, R, out_ch) bytes (a pure host function; -1 for bad arguments).
 * stats: HOST int64 [4] or NULL <- {live, total} points of the coarse pass, {live, total} of the fine pass (0, 0 without one). */
int64_t nerf_amd_render_rays_culled_workspace(const nerf_amd_render_cfg *cfg, int64_t R, int32_t out_ch);
int     nerf_amd_render_rays_culled(const nerf_amd_render_cfg *cfg, const nerf_amd_model *coarse, const nerf_amd_model *fine,
                                    const nerf_amd_render_io *io, int64_t R, const nerf_amd_occupancy_grid *grid,
                                    int64_t *stats, void *stream);

/* Image output stage: utils.to8b (utils.py:30) as used by Renderer.render_from_batch_poses
 * (render_utils.py:312): out[i] = uint8(255 * clip(x[i], 0, 1)), truncating; NaN -> 0.
 * x [n] fp32 DEVICE (16-byte aligned), out [n] uint8 DEVICE (4-byte aligned). */
int nerf_amd_to8b(const float *x, int64_t n, uint8_t *out, void *stream);

/* utils.img2mse (utils.py:24; the loss of main.py:93-98): out[0] = mean((x - y)^2) over n fp32 DEVICE values.
 * One launch for n <= 16384 (a training batch); beyond that `partials` (256 floats, DEVICE) is required and a second
 * tiny launch sums the per-block partials in a fixed order.  _backward: gx = g[0] * 2 (x - y) / n, gy = -gx (either may
 * be NULL), g = the DEVICE scalar gradient of the loss. */
int nerf_amd_img2mse(const float *x, const float *y, int64_t n, float *out, float *partials, void *stream);
int nerf_amd_img2mse_backward(const float *x, const float *y, int64_t n, const float *g, float *gx, float *gy, void *stream);

/* Renderer.render(rays=...) batch assembly (render_utils.py:205-222) in one launch: out[i] = [rays_o[i] | rays_d[i] |
 * near | far | viewdir_src[i] / |viewdir_src[i]|]; viewdir_src NULL -> 8 columns, else 11.  All [n, 3] fp32 DEVICE,
 * contiguous.  (The c2w path has nerf_amd_make_rays.) */
int nerf_amd_assemble_rays(const float *rays_o, const float *rays_d, const float *viewdir_src, int64_t n, float near,
                           float far, float *out, void *stream);

/* Optimizer step of the training loop (main.py:104 on the torch.optim.Adam of utils.py:163-172): Adam for
 * n parameter tensors in one launch.  params / grads / exp_avg / exp_avg_sq: HOST arrays of n DEVICE pointers
 * to fp32 tensors of numel[i] elements (4-byte aligned; any n).  Per element, in fp32 and in the order of
 * torch/optim/adam.py _single_tensor_adam:
 *   g += weight_decay p (if != 0);  m += (1 - beta1)(g - m);  v = v beta2 + (1 - beta2) g g;
 *   p -= (lr / bias_correction1) * m / (sqrt(v) / sqrt(bias_correction2) + eps)
 * with bias_correction{1,2} = 1 - beta{1,2}^step evaluated in double from `step` (>= 1, the count INCLUDING
 * this step).  amsgrad / maximize are not provided. */
int nerf_amd_adam_step(int32_t n, float *const *params, const float *const *grads, float *const *exp_avg,
                       float *const *exp_avg_sq, const int64_t *numel, int64_t step, double lr, double beta1,
                       double beta2, double eps, double weight_decay, void *stream);

/* The same update for a CAPTURED training step (a HIP graph replays the arguments it was captured with, so nothing that
 * changes per step may be an argument): the step count *step_dev (int64, DEVICE; advanced by one on every execution) and
 * the learning rate *lr_dev (double, DEVICE; the caller rewrites it between replays for main.py:108-112's decay) live in
 * device memory; scalars_dev is 2 floats of DEVICE scratch.  n <= 64. */
int nerf_amd_adam_step_device(int32_t n, float *const *params, const float *const *grads, float *const *exp_avg,
                              float *const *exp_avg_sq, const int64_t *numel, int64_t *step_dev, const double *lr_dev,
                              double beta1, double beta2, double eps, double weight_decay, float *scalars_dev, void *stream);

/* ------------------------------------------------------------------------
 * Measurement hook (bench.py): while enabled, every field-MLP launch is
 * bracketed by hipEvents on its own stream.  nerf_amd_profile_collect waits for
 * the recorded events and returns, per class (0 = fp32 kernel, 1 = fused bf16
 * kernel, 2 = split-precision kernel), the number of launches, the summed device time in milliseconds and
 * the summed number of points, then forgets them.
 * ------------------------------------------------------------------------ */
int nerf_amd_profile_enable(int on);
/* Tuning knobs for A/B measurements (results are identical for every setting).
 * key 0: weight-pipeline shape of the fused bf16 kernel (0 = default; see mlp_bf16.hip launch_one).
 *        Values 50..58 once chose earlier generations of the weight-gradient launcher; they are still accepted and do nothing.
 * key 1: route of nerf_amd_density_value_grad (0 = default: the fused kernel where it covers the model, 1 = always two launches).
 * key 2: where NERF_AMD_PREC_BF16 runs the folded stream (NERF_AMD_COPY_BF16_FOLD) of a view-branch model:
 *        0 = default: in the no-grad render path (nerf_amd_render_batch and the render calls built on the same stages);
 *            nerf_amd_nerf_forward stays unfolded and bit-equal to the training forward;
 *        1 = nowhere (A/B leg: the unfolded kernels everywhere);
 *        2 = in nerf_amd_nerf_forward too (tests, tools/mlp_ab.py).
 * key 3: the colour branch (views_linears.0, rgb) of 16-sample blocks whose sigmas are all <= 0, in the folded render kernels:
 *        0 = default: not computed where a render hands out no raw and adds no sigma noise (nerf_amd_render_rays / _chunks /
 *            _batch with io->raw, io->noise0 and io->noise1 NULL and use_noise 0): such samples have weight exactly 0, the maps
 *            are bit-identical; everything else (raw to the caller, noise, nerf_amd_nerf_forward, nerf_amd_field_points, the
 *            culled renders, training, density queries, fp32 and fp32_split) computes every sample;
 *        1 = never (A/B leg). */
int nerf_amd_set_tuning(int key, int value);
int nerf_amd_profile_collect(int64_t launches[3], double total_ms[3], double total_points[3]);

#ifdef __cplusplus
}
#endif
#endif /* NERF_AMD_H */
