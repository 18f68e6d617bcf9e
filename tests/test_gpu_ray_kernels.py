"""The per-ray kernels of csrc/render.hip under every gradient (-m gpu): raw2outputs backward, get_rays backward (the
pose gradient), ndc_rays backward, and the dynamic-LDS range above the 64-KiB default of composite_bwd_kernel,
sample_pdf_kernel, resample_kernel and mid_stage_kernel.

The reference is the oracle's own function run in float64 (O.raw2outputs, O.get_rays and O.ndc_rays promote cleanly), so
a disagreement has a judge.  The gradient gate is relative to what fp32 autograd of the same expression achieves:

    per ray, normwise:  |g_gpu - g64| <= 4 |g32 - g64| + 2^-20 |g64|

(raw2outputs adds to |g64| the size of the terms that cancel in dL/dalpha, see cancellation_scale; ndc_rays takes 64 for
4: the docstrings of the two tests give the measured reasons)

plus exact zeros where the gradient is 0 by construction (channels >= 4, samples with sigma <= 0, one-sample rays), and
fp32 autograd's NaN/Inf pattern element by element (autograd is the specification of what a NaN upstream gradient
reaches).  The measured share of the gate each case uses, and its ratio |g_gpu - g64| / |g32 - g64|, go to the parity report
(test_gpu_parity.report).

NERF_AMD_FUZZ_SCALE / NERF_AMD_FUZZ_SEED scale the sweeps and pick another family of cases, as in test_gpu_fuzz.py.
"""
import os

import numpy as np
import pytest
import torch

import test_gpu_parity as P
from nerf_shared_amd import synth

pytestmark = pytest.mark.gpu

dev = P.dev
O = P.O

SCALE = max(1, int(os.environ.get("NERF_AMD_FUZZ_SCALE", "1")))
FAMILY = int(os.environ.get("NERF_AMD_FUZZ_SEED", "0"))

GATE_FACTOR, GATE_FLOOR = 4.0, 2.0 ** -20
FLT_MIN = 2.0 ** -126


def _rng(base, i):
    return np.random.default_rng(base + i + 1000003 * FAMILY)


# Dynamic LDS of the per-ray kernels (render.hip: RAYS_PER_WG, LDS_PER_CU, composite_bwd_lds_bytes, sample_pdf_lds_bytes,
# resample_lds_bytes).  Every refused call below checks that the library's message quotes the same byte count, which ties
# this restatement to the C++ one.
RAYS_PER_WG, LDS_DEFAULT, LDS_PER_CU = 4, 64 * 1024, 160 * 1024


def _pow2_at_least(n):
    p = 2
    while p < n:
        p <<= 1
    return p


def composite_bwd_lds_bytes(S):
    return RAYS_PER_WG * 3 * S * 4


def sample_pdf_lds_bytes(n_bins):
    return RAYS_PER_WG * 2 * n_bins * 4


def resample_lds_bytes(Nc, Ni, with_composite):
    return RAYS_PER_WG * ((Nc if with_composite else 0) + 2 * (Nc - 1) + _pow2_at_least(Nc) + _pow2_at_least(Ni)) * 4


def _first_above(f, limit):
    """Smallest n >= 2 with f(n) > limit (f non-decreasing)."""
    n = 2
    while f(n) <= limit:
        n += 1
    return n


def _refused(fn, nbytes):
    from nerf_shared_amd._lib import NerfAmdError
    with pytest.raises(NerfAmdError, match="needs %d bytes of LDS" % nbytes):
        fn()


# ---------------------------------------------------------------------------------------------------------------------
# the gradient gate
# ---------------------------------------------------------------------------------------------------------------------
def gradient_gate(label, gpu, g32, g64, rows, factor=GATE_FACTOR, scale=None, zeros=None):
    """Asserts the module's gate on one gradient, `rows` rays (any trailing shape).  Returns (how much of the gate the
    worst ray uses: max |g_gpu - g64| / bound, the worst |g_gpu - g64| / |g32 - g64| over rays where the factor's term
    of the bound is the larger one).  `scale` [rows]: the size of the terms that cancel
    in the gradient (see cancellation_scale), added to |g64| in the floor.  `zeros`: where the gradient is 0 by construction
    (default: where both autograds are exactly 0)."""
    gpu, g32, g64 = (t.detach().cpu().double().reshape(rows, -1) for t in (gpu, g32, g64))
    nan_g, nan_32 = torch.isnan(gpu), torch.isnan(g32)
    assert torch.equal(nan_g, nan_32), (label, "NaN pattern", int((nan_g != nan_32).sum()),
                                        torch.nonzero(nan_g != nan_32)[:8].tolist())
    inf_g, inf_32 = torch.isinf(gpu), torch.isinf(g32)
    assert torch.equal(inf_g, inf_32) and torch.equal(gpu[inf_g], g32[inf_32]), (label, "Inf pattern")
    # A 0 that autograd reaches by cancellation (disp of a ray with one live sample: depth / acc = z; acc of the sample in
    # front of an opaque last one: T_s - w_{s+1} / (1 - alpha_s) = 0) is a rounding residue in another evaluation order;
    # the norm gate covers those.
    zero = ((g64 == 0) & (g32 == 0)) if zeros is None else zeros.reshape(rows, -1)
    assert bool((gpu[zero] == 0).all()), (label, "not exactly 0 where autograd is", torch.nonzero(zero & (gpu != 0))[:8].tolist())
    fin = torch.isfinite(g32) & torch.isfinite(g64)
    e_gpu = torch.where(fin, gpu - g64, 0.).norm(dim=1)
    e_32 = torch.where(fin, g32 - g64, 0.).norm(dim=1)
    ref = torch.where(fin, g64, 0.).norm(dim=1)
    # (+ FLT_MIN: below fp32's normal range a product keeps no relative precision; rays whose gradient is ~1e-44 were met)
    floor = GATE_FLOOR * (ref if scale is None else ref + scale) + FLT_MIN
    bound = factor * e_32 + floor
    bad = e_gpu > bound
    assert not bool(bad.any()), (label, "rays", torch.nonzero(bad)[:8].flatten().tolist(), float(e_gpu[bad].max()),
                                 float(bound[bad].max()), float(ref[bad].max()))
    by_factor = factor * e_32 >= floor
    ratio = float((e_gpu[by_factor] / e_32[by_factor]).max()) if bool(by_factor.any()) else 0.0
    return float((e_gpu / bound).max()), ratio


# ---------------------------------------------------------------------------------------------------------------------
# 1. raw2outputs backward (composite_bwd_kernel) against fp64 autograd of O.raw2outputs
# ---------------------------------------------------------------------------------------------------------------------
OUT_NAMES = ("rgb", "disp", "acc", "weights", "depth")


def raw2outputs_inputs(rng, R, S, ch, scale, noise_std):
    """raw [R,S,ch], z [R,S], rays_d [R,3] (|d| in 0.5..3), noise [R,S] (the pytest draw x std, or None).  Where R >= 5
    rays 0..4 are planted: empty, opaque from the first sample, sigma exactly 0 at every third sample, sigma > 0 with
    alpha underflowing to 0, depth / acc below 1e-10 (the clamp of disp)."""
    raw = (rng.normal(size=(R, S, ch)) * scale).astype(np.float32)
    z = np.sort(rng.uniform(0.1, 9, size=(R, S)), -1).astype(np.float32)
    d = rng.normal(size=(R, 3))
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True) * rng.uniform(0.5, 3, size=(R, 1))).astype(np.float32)
    noise = (O.pytest_uniform([R, S]) * noise_std).numpy() if noise_std > 0 else None
    nz = noise if noise is not None else np.zeros((R, S), np.float32)
    if R >= 5:
        raw[0, :, 3] = -2.0 - noise_std                                  # empty: sigma + noise < 0 everywhere, acc 0, disp NaN
        z[1, 1:] += 1.5                                                  # opaque: first interval >= 0.75, 30 * 0.75 -> alpha = 1.0f
        raw[1, :, 3] = 30.0
        raw[2, ::3, 3] = -nz[2, ::3]                                     # sigma + noise exactly 0: the ReLU boundary
        z[3] = (1e-3 + 1e-9 * np.arange(S)).astype(np.float32)          # intervals of ~1e-9: sigma * dist < 2^-25, alpha = 0
        raw[3, :, 3] = 1e-20
        raw[3, -1, 3] = -2.0 - noise_std                                 # (the 1e10 tail must not make it opaque)
        z[4] = np.linspace(0.0, 5e-11, S).astype(np.float32)            # depth / acc < 1e-10: disp's clamp branch
        raw[4, :, 3] = np.abs(raw[4, :, 3]) + 1.0
    if S >= 4:
        z[:, S // 2] = z[:, S // 2 - 1]                                  # a zero-length interval in the middle
    if S >= 3 and rng.random() < 0.5:
        z[:, -1] = z[:, -2]                                              # and one at the end
    return raw, z, d, noise


def cancellation_scale(outs, sel, coef, raw, z, d, noise):
    """Per ray (fp64), the size of the two terms whose difference is dL/dalpha_s = v_s T_s - sum_{k>s} v_k w_k / (1 - alpha_s
    + 1e-10), carried to sigma and to |rays_d|: the norm over the samples of dist_s exp(-sigma_s dist_s) (|v_s| T_s +
    sum_{k>s} |v_k| w_k / (1 - alpha_s + 1e-10)), and the sum over the samples of the same with sigma_s dz_s for dist_s;
    samples with sigma_s <= 0 contribute nothing (relu's derivative is 0 there).  Each sample's share is weighted by
    1 + sigma_s dist_s, the condition number of exp(-sigma_s dist_s): an alpha that rounds to 1 sits at sigma dist ~ 20-30,
    where one ulp of dist (|rays_d| is summed in another order than torch.norm's) moves the gradient by 25 ulps (measured:
    4e-6 of |g64| on such a ray at scale 4, fp32 autograd 1e-6).  Where the two nearly cancel (the acc
    of an opaque ray: the exact gradient is T_end / (1 - alpha_s), 1e-10 and below), fp32 autograd can land within 1e-12
    of it, and the kernel (same formula, the sum of the later terms in fp64, rounded once) a few ulps of these terms away:
    measured on an MI355X up to 4e3 x |g32 - g64| on such rays (family 0, scale 1), which the factor-4 gate alone
    refused.  A wrong term is off by its own size, far above 2^-20 of this scale."""
    w = outs[3]
    if w.shape[1] == 0:
        return torch.zeros(w.shape[0], dtype=torch.float64), torch.zeros(w.shape[0], dtype=torch.float64)
    v = torch.autograd.grad([outs[k] for k in sel], [w], [coef[k] for k in sel], retain_graph=True)[0].detach().abs()
    if 1 in sel:                       # v itself cancels under disp: dL/dw_s = dL/dq (z_s - q) / acc, q = depth / acc
        disp, acc, q = outs[1].detach(), outs[2].detach(), (outs[4] / outs[2]).detach()
        gq = torch.where(q > 1e-10, coef[1] * disp * disp, torch.zeros_like(q)).abs()
        v = v + (gq / acc)[:, None] * (z.abs() + q.abs()[:, None])
    dz = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], 1e10)], -1)
    dist = dz * torch.norm(d.detach(), dim=-1, keepdim=True)
    sig = torch.relu(raw.detach()[..., 3] + (noise if noise is not None else 0.0))
    e = torch.exp(-sig * dist)
    x = e + 1e-10                                                        # 1 - alpha + 1e-10
    T = torch.cumprod(torch.cat([torch.ones_like(e[:, :1]), x], -1), -1)[:, :-1]
    u = v * (1.0 - e) * T                                                # |v_k| w_k
    later = torch.flip(torch.cumsum(torch.flip(u, [-1]), -1), [-1]) - u  # sum over k > s
    # relu's backward: a sample with sigma <= 0 contributes exactly 0 and cancels nothing.  (1 + sigma dist): exp's condition
    # number, an ulp of sigma * dist moves exp(-sigma dist) by sigma * dist ulps
    t = torch.where(sig > 0, e * (v * T + later / x) * (1.0 + sig * dist), torch.zeros_like(e))
    return torch.nan_to_num((t * dist).norm(dim=1)), torch.nan_to_num((t * sig * dz).sum(1))


def check_raw2outputs_backward(dev, label, rng, R, S, ch, scale, white, noise_std):
    """Six backward passes (each output alone with a random coefficient tensor, then all five) through Renderer.raw2outputs
    against fp64 and fp32 autograd of O.raw2outputs on the same inputs and noise.  Returns the worst gate ratios."""
    _, render_utils, _ = P.amd()
    raw, z, d, noise = raw2outputs_inputs(rng, R, S, ch, scale, noise_std)
    shapes = ((R, 3), (R,), (R,), (R, S if S > 1 else 0), (R,))
    coef = [torch.from_numpy(rng.normal(size=s).astype(np.float32)) for s in shapes]
    passes = [[k] for k in range(5)] + [list(range(5))]

    def grads(outs, raw_t, d_t, c):
        res = []
        for sel in passes:
            if raw_t.dtype == torch.float64 and not raw_t.is_cuda:
                scales.append(cancellation_scale(outs, sel, c, raw_t, torch.from_numpy(z).double(), d_t,
                                                 None if noise is None else torch.from_numpy(noise).double()))
            g = torch.autograd.grad([outs[k] for k in sel], [raw_t, d_t], [c[k] for k in sel], retain_graph=True,
                                    allow_unused=True)
            res.append([torch.zeros_like(t) if gi is None else gi for gi, t in zip(g, (raw_t, d_t))])
        return res

    ref, scales = {}, []
    for dt in (torch.float64, torch.float32):
        raw_c = torch.from_numpy(raw).to(dt).requires_grad_(True)
        d_c = torch.from_numpy(d).to(dt).requires_grad_(True)
        n_c = torch.from_numpy(noise).to(dt) if noise is not None else None
        outs = O.raw2outputs(raw_c, torch.from_numpy(z).to(dt), d_c, white, n_c)
        ref[dt] = grads(outs, raw_c, d_c, [c.to(dt) for c in coef])
    r = render_utils.Renderer(**dict(P.BASE, white_bkgd=white, raw_noise_std=noise_std))
    raw_g = torch.from_numpy(raw).to(dev).requires_grad_(True)
    d_g = torch.from_numpy(d).to(dev).requires_grad_(True)
    outs = r.raw2outputs(raw_g, torch.from_numpy(z).to(dev), d_g, pytest=noise is not None)
    got = grads(outs, raw_g, d_g, [c.to(dev) for c in coef])
    worst = {}
    # zero by construction: channels >= 4, sigma + noise <= 0 (relu), every entry of a one-sample ray, rgb channels when rgb
    # is not in the loss
    sig = torch.from_numpy(raw[..., 3] + (noise if noise is not None else 0.0))
    zr = torch.zeros(R, S, ch, dtype=torch.bool)
    zr[..., 4:] = True
    zr[..., 3] = sig <= 0
    if S == 1:
        zr[:] = True
    zeros_no_rgb = zr.clone()
    zeros_no_rgb[..., :3] = True
    zeros = (zr, torch.full((R, 3), S == 1))
    for p, sel in enumerate(passes):
        name = "+".join(OUT_NAMES[k] for k in sel)
        for j, key in enumerate(("g_raw", "g_rays_d")):
            use, ratio = gradient_gate("%s %s %s" % (label, name, key), got[p][j], ref[torch.float32][p][j],
                                       ref[torch.float64][p][j], R, scale=scales[p][j],
                                       zeros=zeros[j] if j or 0 in sel else zeros_no_rgb)
            worst[key + "_use"] = max(worst.get(key + "_use", 0.0), use)
            worst[key + "_ratio"] = max(worst.get(key + "_ratio", 0.0), ratio)
    return worst


R2O_RAYS = (1, 2, 3, 5, 63, 64, 65, 300)
R2O_SAMPLES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 192, 513, 1500)


def draw_raw2outputs_case(i):
    rng = _rng(31000, i)
    S = int(rng.choice(R2O_SAMPLES))
    R = int(rng.choice([r for r in R2O_RAYS if r * S <= 100000]))      # the CPU oracle stays cheap at large S
    if i % 3 == 0:
        R = max(R, 5)                                                    # every third case carries the planted rays
    ch = int(rng.choice([4, 5, 9]))
    scale = float(rng.choice([0.3, 3.0, 30.0]))
    white, noise_std = bool(rng.random() < 0.5), float(rng.choice([0.0, 0.7]))
    return rng, R, S, ch, scale, white, noise_std


@pytest.mark.parametrize("i", range(24 * SCALE))
def test_raw2outputs_backward_against_fp64_autograd(dev, i):
    """composite_bwd_kernel across one, two and many 64-sample chunks (the suffix-sum carry), the 1e10 last interval,
    zero-length intervals, channels >= 4, one-sample rays, sigma noise, non-unit rays_d, and the planted rays (empty,
    opaque, sigma exactly 0, underflowing alpha, clamped disp), one output at a time and all together.

    The gate's floor adds the size of the terms that cancel in dL/dalpha to |g64|: see cancellation_scale for why and for
    what was measured on the GPU without it."""
    rng, R, S, ch, scale, white, noise_std = draw_raw2outputs_case(i)
    label = "r2o%d R=%d S=%d ch=%d scale=%g white=%d noise=%g" % (i, R, S, ch, scale, white, noise_std)
    worst = check_raw2outputs_backward(dev, label, rng, R, S, ch, scale, white, noise_std)
    P.report("ray_r2o_bwd_%03d" % i, dict(worst, R=R, S=S, ch=ch))


def test_raw2outputs_backward_reads_rays_d_with_the_batch_stride(dev):
    """render_rays passes rays_d as columns 3:6 of the [R, 11] ray batch (stride 11); the Python wrapper always hands the
    kernel a contiguous copy.  Both must give the same bits."""
    from nerf_shared_amd import _lib
    lib = _lib.lib
    rng = _rng(32000, 0)
    R, S, ch = 70, 130, 5
    raw, z, d, noise = raw2outputs_inputs(rng, R, S, ch, 3.0, 0.7)
    rays = torch.from_numpy(rng.normal(size=(R, 11)).astype(np.float32))
    rays[:, 3:6] = torch.from_numpy(d)
    t = {k: torch.from_numpy(v).to(dev) for k, v in dict(raw=raw, z=z, d=d, noise=noise).items()}
    rays = rays.to(dev)
    g = [torch.from_numpy(rng.normal(size=s).astype(np.float32)).to(dev) for s in ((R, 3), (R,), (R,), (R,), (R, S))]
    res = []
    for dptr, stride in ((rays[:, 3:6].data_ptr(), 11), (t["d"].data_ptr(), 3)):
        g_raw = torch.full((R, S, ch), 7.0, device=dev)
        g_d = torch.full((R, 3), 7.0, device=dev)
        for white in (0, 1):
            _lib.check(lib.nerf_amd_raw2outputs_backward(t["raw"].data_ptr(), ch, t["z"].data_ptr(), dptr, stride,
                                                         t["noise"].data_ptr(), R, S, white, g[0].data_ptr(), g[1].data_ptr(),
                                                         g[2].data_ptr(), g[3].data_ptr(), g[4].data_ptr(), g_raw.data_ptr(),
                                                         g_d.data_ptr(), _lib.stream_of(dev)), "nerf_amd_raw2outputs_backward")
            torch.cuda.synchronize()
            res.append((g_raw.clone(), g_d.clone()))
    for (a_raw, a_d), (b_raw, b_d) in zip(res[:2], res[2:]):
        assert torch.equal(a_raw.view(torch.int32), b_raw.view(torch.int32))
        assert torch.equal(a_d.view(torch.int32), b_d.view(torch.int32))
    assert bool(torch.isnan(res[0][1][0]).all())                         # the empty ray, disp in the loss: autograd's NaN


# ---------------------------------------------------------------------------------------------------------------------
# 2. the LDS opt-in range (64 KiB < bytes <= 160 KiB), both edges
# ---------------------------------------------------------------------------------------------------------------------
def test_lds_byte_counts_of_the_quoted_edges():
    """The sizes the tests below run at, derived from the restated byte counts (checked against the library's own
    through the refusal messages)."""
    assert _first_above(composite_bwd_lds_bytes, LDS_DEFAULT) == 1366
    assert _first_above(composite_bwd_lds_bytes, LDS_PER_CU) - 1 == 3413 and composite_bwd_lds_bytes(3413) == 163824
    assert _first_above(sample_pdf_lds_bytes, LDS_DEFAULT) == 2049 and sample_pdf_lds_bytes(2048) == 65536
    assert _first_above(sample_pdf_lds_bytes, LDS_PER_CU) - 1 == 5120 and sample_pdf_lds_bytes(5120) == LDS_PER_CU
    assert resample_lds_bytes(1024, 64, False) <= LDS_DEFAULT < resample_lds_bytes(1025, 64, False)
    assert resample_lds_bytes(2049, 2048, False) == LDS_PER_CU < resample_lds_bytes(2049, 2049, False)
    assert LDS_DEFAULT < resample_lds_bytes(1024, 1024, True) and resample_lds_bytes(2048, 2048, True) <= LDS_PER_CU


COMPOSITE_LDS_S = (_first_above(composite_bwd_lds_bytes, LDS_DEFAULT), 2048, _first_above(composite_bwd_lds_bytes, LDS_PER_CU) - 1)


@pytest.mark.parametrize("S", COMPOSITE_LDS_S)
def test_raw2outputs_backward_in_the_lds_opt_in_range(dev, S):
    rng = _rng(33000, S)
    R = 4 + S % 5
    worst = check_raw2outputs_backward(dev, "r2o lds S=%d" % S, rng, R, S, int(rng.choice([4, 9])), 3.0, bool(S % 2),
                                       0.7 if S % 2 == 0 else 0.0)
    P.report("ray_r2o_bwd_lds_%d" % S, dict(worst, R=R, S=S))


def test_raw2outputs_backward_beyond_the_lds_is_refused(dev):
    _, render_utils, _ = P.amd()
    S = _first_above(composite_bwd_lds_bytes, LDS_PER_CU)
    r = render_utils.Renderer(**P.BASE)
    raw = torch.randn(4, S, 4, device=dev, requires_grad=True)
    z = torch.rand(4, S, device=dev).sort(-1)[0]
    rgb = r.raw2outputs(raw, z, torch.randn(4, 3, device=dev))[0]
    _refused(lambda: rgb.sum().backward(), composite_bwd_lds_bytes(S))
    assert raw.grad is None


def _sample_pdf_case(rng, R, nb, N, det):
    bins = np.sort(rng.uniform(2, 6, size=(R, nb)).astype(np.float32), -1)
    w = rng.uniform(0, 1, size=(R, nb - 1)).astype(np.float32) ** float(rng.choice([1.0, 4.0]))
    for r_ in range(R):                                                  # most bins empty: the mass sits in well-conditioned bins
        w[r_, rng.random(nb - 1) < [0.0, 0.95, 0.99][r_ % 3]] = 0.0
    w[-1] = 0.0                                                          # an all-zero row: uniform pdf
    return bins, w


def check_sample_pdf_like_the_fuzz(got, bins_t, w_t, u, label):
    """The gates of test_gpu_fuzz.test_random_sample_pdf_shapes."""
    R, N = got.shape
    nb = bins_t.shape[1]
    ref = O.sample_pdf(bins_t, w_t, N, u=u.contiguous())
    assert got.shape == ref.shape
    well = P.pdf_denominators(bins_t, w_t, u) > 1e-3
    d = (got - ref).abs().numpy()
    assert well.sum() > N, (label, "too few well-conditioned samples to mean anything", int(well.sum()))
    bad = int((d[well] >= 2e-5).sum())
    assert bad <= max(1, int(1e-3 * well.sum())), (label, bad, float(d[well].max()))
    widest = np.diff(bins_t.numpy(), axis=-1).max(-1)[:, None] if nb > 1 else np.zeros((R, 1), np.float32)
    assert (d <= widest * 1.001 + 4e-6).all(), (label, float(d.max()))
    return ref


SAMPLE_PDF_LDS_BINS = (2048, _first_above(sample_pdf_lds_bytes, LDS_DEFAULT), 4000, _first_above(sample_pdf_lds_bytes, LDS_PER_CU) - 1)


@pytest.mark.parametrize("nb", SAMPLE_PDF_LDS_BINS)
def test_sample_pdf_in_the_lds_opt_in_range(dev, nb):
    _, _, utils = P.amd()
    rng = _rng(34000, nb)
    R, N = 7, 257
    for det in (True, False):
        bins, w = _sample_pdf_case(rng, R, nb, N, det)
        bins_t, w_t = torch.from_numpy(bins), torch.from_numpy(w)
        got = utils.sample_pdf(bins_t.to(dev), w_t.to(dev), N, det=det, pytest=not det).cpu()
        u = O.pytest_u_for_sample_pdf(R, N, det) if not det else torch.linspace(0., 1., N).expand(R, N)
        check_sample_pdf_like_the_fuzz(got, bins_t, w_t, u, "sample_pdf nb=%d det=%d" % (nb, det))


def test_sample_pdf_beyond_the_lds_is_refused(dev):
    _, _, utils = P.amd()
    nb = _first_above(sample_pdf_lds_bytes, LDS_PER_CU)
    bins = torch.rand(4, nb, device=dev).sort(-1)[0]
    _refused(lambda: utils.sample_pdf(bins, torch.rand(4, nb - 1, device=dev), 16, det=True), sample_pdf_lds_bytes(nb))


def _resample(dev, zt, wt, ut, t_lin, R, nc, ni):
    from nerf_shared_amd import _lib
    z_fine = torch.empty(R, nc + ni, device=dev)
    z_std = torch.empty(R, device=dev)
    _lib.check(_lib.lib.nerf_amd_resample(zt.data_ptr(), wt.data_ptr(), _lib.ptr(ut), t_lin.data_ptr(), R, nc, ni,
                                          z_fine.data_ptr(), z_std.data_ptr(), _lib.stream_of(dev)), "nerf_amd_resample")
    return z_fine, z_std


# (1025, 64): the first coarse count past the default; (2048, 2048); (2049, 2048): exactly the CU's 160 KiB
RESAMPLE_LDS_PAIRS = ((_first_above(lambda n: resample_lds_bytes(n, 64, False), LDS_DEFAULT), 64), (2048, 2048), (2049, 2048))


@pytest.mark.parametrize("nc,ni", RESAMPLE_LDS_PAIRS)
def test_resample_in_the_lds_opt_in_range(dev, nc, ni):
    """nerf_amd_resample (the training path's resampling) at coarse counts that need the opt-in, against the library's
    sample_pdf + torch.sort bit for bit (test_gpu_parity.test_resample_stage_against_sample_pdf_and_torch_sort) and the
    oracle's sample_pdf + torch.sort with the fuzz's gates."""
    from nerf_shared_amd import _lib
    assert LDS_DEFAULT < resample_lds_bytes(nc, ni, False) <= LDS_PER_CU
    rng = _rng(35000, nc + ni)
    R = 9                                                                # the last workgroup: one live wave, three padding waves
    for case in ("sorted", "random_u"):
        z = np.sort(rng.uniform(2, 6, size=(R, nc)).astype(np.float32), -1)
        w = rng.uniform(0, 1, size=(R, nc)).astype(np.float32) ** 4
        w[:, 1:-1][rng.random((R, nc - 2)) < 0.97] = 0.0
        w[5] = 0.0                                                       # all-zero row: uniform pdf
        u = None if case == "sorted" else rng.uniform(0, 1, size=(R, ni)).astype(np.float32)
        zt, wt = torch.from_numpy(z).to(dev), torch.from_numpy(w).to(dev)
        ut = None if u is None else torch.from_numpy(u).to(dev)
        t_lin = torch.linspace(0., 1., ni, device=dev)
        z_fine, z_std = _resample(dev, zt, wt, ut, t_lin, R, nc, ni)
        zm, wm = (.5 * (zt[:, 1:] + zt[:, :-1])).contiguous(), wt[:, 1:-1].contiguous()
        samples = torch.empty(R, ni, device=dev)
        _lib.check(_lib.lib.nerf_amd_sample_pdf(zm.data_ptr(), wm.data_ptr(), _lib.ptr(ut), t_lin.data_ptr(), R, nc - 1, ni,
                                                samples.data_ptr(), _lib.stream_of(dev)), "nerf_amd_sample_pdf")
        assert torch.equal(z_fine, torch.sort(torch.cat([zt, samples], -1), -1)[0]), case
        P.close(z_std, torch.std(samples, -1, unbiased=False), atol=2e-6)
        u_ref = torch.from_numpy(u) if u is not None else torch.linspace(0., 1., ni).expand(R, ni)
        ref = check_sample_pdf_like_the_fuzz(samples.cpu(), zm.cpu(), wm.cpu(), u_ref, "resample %d+%d %s" % (nc, ni, case))
        z_ref = torch.sort(torch.cat([torch.from_numpy(z), ref], -1), -1)[0]
        bin_w = np.diff(zm.cpu().numpy(), axis=-1).max(-1)[:, None]
        assert ((z_fine.cpu() - z_ref).abs().numpy() <= bin_w * 1.001 + 4e-6).all(), case


def test_resample_beyond_the_lds_is_refused(dev):
    nc = 2049
    ni = _first_above(lambda n: resample_lds_bytes(nc, n, False), LDS_PER_CU)
    R = 4
    zt = torch.rand(R, nc, device=dev).sort(-1)[0]
    wt = torch.rand(R, nc, device=dev)
    t_lin = torch.linspace(0., 1., ni, device=dev)
    _refused(lambda: _resample(dev, zt, wt, None, t_lin, R, nc, ni), resample_lds_bytes(nc, ni, False))


SMALL_VD = dict(D=2, W=32, output_ch=5, skips=[], use_viewdirs=True, multires=10, multires_views=4)


@pytest.mark.parametrize("n", (1024, 2048))
def test_render_rays_in_the_lds_opt_in_range_against_the_oracle(dev, n):
    """mid_stage_kernel (compositing + resampling in one launch, the inference render_rays) at n + n samples, staged
    against the oracle on a small model on the exact-fp32 kernel."""
    assert LDS_DEFAULT < resample_lds_bytes(n, n, True) <= LDS_PER_CU
    cfg = dict(P.BASE, N_samples=n, N_importance=n)
    H = W = 400
    K = synth.lego_intrinsics(H, W)
    idx = np.sort(_rng(36000, n).choice(H * W, size=6, replace=False))
    batch = P.oracle_batch(cfg, H, W, K, synth.pose_spherical(37.0), idx)
    out = P.staged_check(dev, cfg, SMALL_VD, batch, (3, 4, 3.0), False, "lds %d+%d" % (n, n), "fp32")
    P.report("ray_lds_render_%d" % n, out)


# ---------------------------------------------------------------------------------------------------------------------
# 3. get_rays backward (the pose gradient, get_rays_bwd_kernel)
# ---------------------------------------------------------------------------------------------------------------------
def _oracle_pose_grad(H, W, K, c2w, g_o, g_d):
    c = torch.as_tensor(np.asarray(c2w, np.float64)).clone().requires_grad_(True)
    ro, rd = O.get_rays(H, W, K, c)
    ((ro * g_o.cpu().double()).sum() + (rd * g_d.cpu().double()).sum()).backward()
    return c.grad


@pytest.mark.parametrize("i", range(12 * SCALE))
def test_get_rays_backward_on_random_cameras(dev, i):
    _, _, utils = P.amd()
    rng = _rng(37000, i)
    H, W = int(rng.integers(1, 91)), int(rng.integers(1, 91))
    fx, fy = rng.uniform(20, 900, size=2)
    K = np.array([[fx, 0, rng.uniform(-0.2, 1.2) * W], [0, fy, rng.uniform(-0.2, 1.2) * H], [0, 0, 1]])
    c2w = synth.pose_spherical(float(rng.uniform(-180, 180)), float(rng.uniform(-80, 10)), float(rng.uniform(1, 6)))
    rows = 3 if i % 2 else 4
    dtype = torch.float64 if i % 4 >= 2 else torch.float32
    pose = torch.from_numpy(np.vstack([c2w, [0, 0, 0, 1]])[:rows]).to(dtype)
    c = pose.to(dev).requires_grad_(True)
    ro, rd = utils.get_rays(H, W, K, c)
    g_o, g_d = torch.randn(H, W, 3, device=dev), torch.randn(H, W, 3, device=dev)
    ((ro * g_o).sum() + (rd * g_d).sum()).backward()
    assert c.grad.dtype == dtype and c.grad.shape == (rows, 4)
    ref = _oracle_pose_grad(H, W, K, pose, g_o, g_d)
    assert P.rel_l2(c.grad, ref) <= 1e-5, (i, H, W, P.rel_l2(c.grad, ref))
    if rows == 4:
        assert bool((c.grad[3] == 0).all())


def test_get_rays_backward_counts_every_selected_pixel_once(dev):
    """An 800 x 800 frame with upstream gradients at a few pixels only (the pose demo's shape: a full frame, a few hundred
    selected rays): the ends of the first wave, block and grid-stride sweep (1024 x 256 pixels) and the first pixel of the
    second sweep, the last pixel, a dozen random ones.  Each entry of the pose gradient is a sum of about 20 terms, gated
    at 1e-6 of the sum of their magnitudes: a dropped or doubled pixel fails."""
    _, _, utils = P.amd()
    rng = _rng(38000, 0)
    H = W = 800
    K = np.array([[1111.0, 0, 380.3], [0, 1050.0, 412.7], [0, 0, 1]])
    pose = torch.from_numpy(np.vstack([synth.pose_spherical(-30.0, -40.0, 4.0), [0, 0, 0, 1]]).astype(np.float32))
    pix = [0, 63, 64, 255, 256, 262143, 262144, H * W - 1]
    pix += [int(p) for p in rng.choice(np.setdiff1d(np.arange(H * W), pix), size=12, replace=False)]
    g_o, g_d = torch.zeros(H * W, 3), torch.zeros(H * W, 3)
    g_o[pix] = torch.from_numpy(rng.normal(size=(len(pix), 3)).astype(np.float32))
    g_d[pix] = torch.from_numpy(rng.normal(size=(len(pix), 3)).astype(np.float32))
    g_o, g_d = g_o.reshape(H, W, 3), g_d.reshape(H, W, 3)
    c = pose.to(dev).requires_grad_(True)
    ro, rd = utils.get_rays(H, W, K, c)
    ((ro * g_o.to(dev)).sum() + (rd * g_d.to(dev)).sum()).backward()
    got = c.grad.cpu().double()
    ref = _oracle_pose_grad(H, W, K, pose, g_o, g_d)
    dirs = O.get_rays(H, W, K, torch.eye(4, dtype=torch.float64))[1].reshape(-1, 3)     # the fp32 directions, exactly
    mag = torch.zeros(4, 4, dtype=torch.float64)
    mag[:3, :3] = g_d.reshape(-1, 3).double().abs().t() @ dirs.abs()
    mag[:3, 3] = g_o.reshape(-1, 3).double().abs().sum(0)
    err = (got - ref).abs()
    assert bool((err[:3] <= 1e-6 * mag[:3]).all()), (err[:3] / mag[:3]).max()
    assert bool((got[3] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# 4. ndc_rays backward (ndc_rays_bwd_kernel)
# ---------------------------------------------------------------------------------------------------------------------
NDC_RAYS = (1, 255, 256, 257, 1000)
NDC_GATE_FACTOR = 64.0                 # see the docstring of test_ndc_rays_backward_on_random_cameras


@pytest.mark.parametrize("i", range(10 * SCALE))
def test_ndc_rays_backward_on_random_cameras(dev, i):
    """ndc_rays_bwd_kernel against fp64 autograd of O.ndc_rays, R across the 256-thread block edge.

    The gate's factor is 64, not the module's 4: the kernel evaluates the closed-form derivative (1 / p_z, its square, t
    folded back through p = o + t d), not autograd's chain of divisions, so on rays with a large t (|d_z| down to 0.05) its
    rounding differs from fp32 autograd's by more than 4x.  Measured on an MI355X (the ratios this test reports, over rays
    where the factor's term of the bound dominates): up to 18.8 x |g32 - g64| in family 0, 22.7 x at NERF_AMD_FUZZ_SCALE=4
    and 33.9 x in family 1 (NERF_AMD_FUZZ_SEED=1); the errors themselves stay near 1e-6 of the gradient.  A wrong term is
    off by its own size, orders of magnitude above this gate."""
    _, _, utils = P.amd()
    rng = _rng(39000, i)
    H, W = int(rng.integers(1, 90)), int(rng.integers(1, 90))
    K = np.array([[rng.uniform(20, 900), 0, rng.uniform(0, W)], [0, rng.uniform(20, 900), rng.uniform(0, H)], [0, 0, 1]])
    c2w = synth.pose_spherical(float(rng.uniform(-180, 180)), float(rng.uniform(-80, 10)), float(rng.uniform(1, 6)))
    ro, rd = O.get_rays(H, W, K, torch.from_numpy(np.asarray(c2w, np.float32)))
    R = NDC_RAYS[i % len(NDC_RAYS)]
    idx = torch.from_numpy(rng.integers(0, H * W, size=R))
    ro, rd = ro.reshape(-1, 3)[idx].clone(), rd.reshape(-1, 3)[idx].clone()
    ro += torch.from_numpy(rng.normal(0, 0.05, size=(R, 3)).astype(np.float32))   # distinct origins
    rd[:, 2] = -rd[:, 2].abs() - 0.05                                                 # forward-facing: d_z away from 0
    focal, near = float(K[0][0]), float(rng.choice([1.0, 0.5]))
    wo, wd = (torch.from_numpy(rng.normal(size=(R, 3)).astype(np.float32)) for _ in range(2))
    o_g, d_g = ro.to(dev).requires_grad_(True), rd.to(dev).requires_grad_(True)
    oo, od = utils.ndc_rays(H, W, focal, near, o_g, d_g)
    ((oo * wo.to(dev)).sum() + (od * wd.to(dev)).sum()).backward()
    ref = {}
    for dt in (torch.float64, torch.float32):
        o_c, d_c = ro.to(dt).requires_grad_(True), rd.to(dt).requires_grad_(True)
        oo_c, od_c = O.ndc_rays(H, W, focal, near, o_c, d_c)
        ((oo_c * wo.to(dt)).sum() + (od_c * wd.to(dt)).sum()).backward()
        ref[dt] = (o_c.grad, d_c.grad)
    worst = {}
    for j, key in enumerate(("g_rays_o", "g_rays_d")):
        worst[key + "_use"], worst[key + "_ratio"] = gradient_gate("ndc%d R=%d %s" % (i, R, key), (o_g.grad, d_g.grad)[j],
                                                                   ref[torch.float32][j], ref[torch.float64][j], R,
                                                                   NDC_GATE_FACTOR)
    P.report("ray_ndc_bwd_%03d" % i, dict(worst, R=R))
