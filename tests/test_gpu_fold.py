"""feature_linear folded into views_linears.0 in the bf16 render kernels (csrc/program.h ST_S16_FOLD, NERF_AMD_COPY_BF16_FOLD,
nerf_amd_set_tuning key 2).

The reference network has no activation between feature_linear and views_linears.0 (nerf.py:110-134), so
    hv = relu(W' h8 + Wv[:, W:] e_dirs + b'),   W' = Wv[:, :W] Wf,   b' = Wv[:, :W] bf + bv
and the no-grad render path evaluates it that way: W' and b' are formed in fp32 from the fp32 parameters when the weights
are packed, and the kernel runs 10.9 % fewer MFMAs per point.  What must hold:
  * the folded stream's layout and the kernels that walk it are right element for element (integer weights: exact);
  * sigma does not move by a bit; rgb is no further from the float64 network than the unfolded kernel's;
  * the render path's z_vals, weights, acc_map, disp_map and sigma do not move by a bit, and rgb_map moves by less than the
    bf16 mode's own error; model(pts, viewdirs) stays unfolded and bit-equal to the training forward;
  * a folded copy never outlives the weights it was made from.
Tuning key 2: 0 = folded in the render path (default), 1 = unfolded everywhere, 2 = folded in model(pts, viewdirs) too -- and
then a missing folded copy is an error, so no test here can pass on the unfolded kernel by accident.

CPU tests (no marker): the preconditions of the exact test, and the host packer's folded stream decoded fragment by fragment.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

os.environ.setdefault("NERF_AMD_QUIET", "1")

import test_gpu_exact_integer as X  # noqa: E402
import test_gpu_parity as P  # noqa: E402
import test_pack_layout as L  # noqa: E402
from nerf_shared_amd import _lib, synth  # noqa: E402
from oracle import nerf_oracle as O  # noqa: E402

gpu = pytest.mark.gpu
lib = _lib.lib
VD = P.VD
FOLDED = ("vd_10_4", "vd_15_6")                 # the view-branch members of the fused family
BF16_FOLDED = _lib.COPY_BF16 | _lib.COPY_BF16_FOLD


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def folded(sd):
    """(W', b') in float64 from a state dict."""
    wf, bf = sd["feature_linear.weight"].double(), sd["feature_linear.bias"].double()
    wv, bv = sd["views_linears.0.weight"].double(), sd["views_linears.0.bias"].double()
    W = wf.shape[0]
    return wv[:, :W] @ wf, wv[:, :W] @ bf + bv


class tuning:
    """nerf_amd_set_tuning(key, value) for a with-block; back to the default afterwards."""

    def __init__(self, key, value):
        self.key, self.value = key, value

    def __enter__(self):
        _lib.check(lib.nerf_amd_set_tuning(self.key, self.value), "set_tuning")

    def __exit__(self, *exc):
        lib.nerf_amd_set_tuning(self.key, 0)


# ================================================================================================ CPU
@pytest.mark.parametrize("name", FOLDED)
def test_integer_weights_fold_exactly(name):
    """The preconditions under which the folded kernel owes the float64 result bit for bit: W' and b' are integers of
    magnitude at most 256 (exact in bf16 and fp32; at most two +-1 per row of Wf and of Wv keep |W'| at 4 or below)."""
    w, b = folded(X.weights(name))
    assert X.is_integer(w) and X.is_integer(b)
    assert float(w.abs().max()) <= 256 and float(b.abs().max()) <= 256
    assert float((w != 0).double().mean()) > 0.005            # not the zero matrix: rows of two to four entries out of 256


def s16_program(arch, fold):
    """Python twin of csrc/program.cpp's s16 order (layer -> pair of 16-row tiles -> segment -> k-step -> tile of the pair):
    [(tensor name, kind, row0, col_base, ks, seg_len, L)] and the bias tiles [(tensor name, row0)].  fold: the ST_S16_FOLD stream."""
    A = X._arch(arch)
    W, ic, icv = A.W, A.input_ch, A.input_ch_views
    KE, KD = L.gen16_ksteps(A.multires), L.gen16_ksteps(A.multires_views)
    E, H = ("gen", 0, ic, KE, A.multires), ("acc", 0, W, 8, 0)
    layers = [("pts_linears.0", W, [E])] + [("pts_linears.%d" % i, W, [H]) for i in range(1, 5)]
    layers += [("pts_linears.5", W, [E, ("acc", ic, W, 8, 0)]), ("pts_linears.6", W, [H]), ("pts_linears.7", W, [H])]
    if not fold:
        layers.append(("feature_linear", W, [H]))
    layers.append(("alpha_linear", 1, [H]))
    layers.append(("FOLD" if fold else "views_linears.0", W // 2, [H, ("gen", W, icv, KD, A.multires_views)]))
    layers.append(("rgb_linear", 3, [("acc", 0, W // 2, 4, 0)]))
    frags, tiles = [], []
    for name, n_out, segs in layers:
        n_tiles = -(-n_out // 16)
        for t in range(0, n_tiles, 2):
            pair = 2 if t + 1 < n_tiles else 1
            tiles += [(name, 16 * (t + u)) for u in range(pair)]
            for kind, col_base, seg_len, nk, mr in segs:
                for ks in range(nk):
                    frags += [(name, kind, 16 * (t + u), col_base, ks, seg_len, mr) for u in range(pair)]
    return frags, tiles


_SLOT_COLS = {}


def slot_cols(kind, ks, mr):
    """[64, 8] input column (inside its segment) of every slot of a fragment, -1 where the slot holds nothing."""
    key = (kind, ks, mr)
    if key not in _SLOT_COLS:
        _SLOT_COLS[key] = np.array([[L.gen16_col(ks, lane >> 4, j, mr) if kind == "gen" else 32 * ks + 16 * (j >> 2) + 4 * (lane >> 4) + (j & 3)
                                     for j in range(8)] for lane in range(64)])           # (acc16_col)
    return _SLOT_COLS[key]


def decode(frags, tensors):
    """The [n, 64, 8] stream a correct packer makes of `frags`: bf16 of the named tensor's element, zero where a slot has none."""
    out = np.zeros((len(frags), 64, 8), np.float32)
    rows16 = np.arange(64) & 15
    for n, (name, kind, row0, col_base, ks, seg_len, mr) in enumerate(frags):
        w = tensors[name]
        c = slot_cols(kind, ks, mr)
        rows = np.broadcast_to((row0 + rows16)[:, None], c.shape)
        ok = (c >= 0) & (c < seg_len) & (rows < w.shape[0])
        out[n][ok] = w[rows[ok], col_base + c[ok]]
    return L.bf16_round(out)


def host_pack(arch, sd, shape):
    names = ["pts_linears.%d" % i for i in range(8)] + ["feature_linear", "alpha_linear", "views_linears.0", "rgb_linear"]
    ws = [np.ascontiguousarray(sd[n + ".weight"], np.float32) for n in names]
    bs = [np.ascontiguousarray(sd[n + ".bias"], np.float32) for n in names]
    a = _lib.make_arch(arch["D"], arch["W"], arch["output_ch"], arch["skips"], arch["use_viewdirs"], arch["multires"],
                       arch["multires_views"], 0)
    n = len(names)
    wp, bp = (ctypes.c_void_p * n)(*[w.ctypes.data for w in ws]), (ctypes.c_void_p * n)(*[b.ctypes.data for b in bs])
    nf, nb = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(lib.nerf_amd_pack_bf16_host(ctypes.byref(a), shape, wp, bp, n, None, ctypes.byref(nf), None, ctypes.byref(nb)), "size query")
    stream, bias = np.zeros(nf.value * 512, np.uint16), np.zeros(nb.value, np.float32)
    _lib.check(lib.nerf_amd_pack_bf16_host(ctypes.byref(a), shape, wp, bp, n, stream.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)),
                                           ctypes.byref(nf), bias.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.byref(nb)), "pack")
    return L.bf16_bits_to_f32(stream).reshape(nf.value, 64, 8), bias.reshape(-1, 16)


@pytest.mark.parametrize("name,integer", [("vd_10_4", True), ("vd_15_6", True), ("vd_10_4", False), ("vd_15_6", False)])
def test_host_packer_folded_stream(name, integer):
    """The host packer's folded stream (shape 20) holds bf16(W') and bf16(Wv[:, W:]) in the slots ST_S16_FOLD names, every
    other layer's fragments where the unfolded stream has them minus the feature layer, zero padding to 192, and the bias
    table b' in the views tiles; the unfolded stream (shape 16) is what it was.  Integer weights: W' is exact.  Random weights:
    the packer sums k ascending in fp32, numpy in float64 -- the bf16 values may differ by one rounding step where W' sits
    on a tie, nowhere else."""
    arch = X.ARCHS[name]
    sd = X.weights(name) if integer else synth.torch_state_dict(3, 3.0, **{**arch, "skips": (4,)})
    sd_np = {k: v.numpy() for k, v in sd.items()}
    w_fold, b_fold = folded(sd)
    W = arch["W"]
    tensors = {k[:-7]: v for k, v in sd_np.items() if k.endswith(".weight")}
    tensors["FOLD"] = np.concatenate([w_fold.numpy(), sd_np["views_linears.0.weight"][:, W:].astype(np.float64)], -1)
    biases = {k[:-5]: v for k, v in sd_np.items() if k.endswith(".bias")}
    biases["FOLD"] = b_fold.numpy()

    plain_frags, plain_tiles = s16_program(arch, False)
    stream16, bias16 = host_pack(arch, sd_np, 16)
    want16 = decode(plain_frags, tensors)
    assert stream16.shape[0] % 192 == 0 and np.array_equal(stream16[:len(plain_frags)], want16)       # the twin reads the program right
    assert not stream16[len(plain_frags):].any()

    frags, tiles = s16_program(arch, True)
    assert len(plain_frags) - len(frags) == 128 and len(plain_tiles) - len(tiles) == 16
    stream, bias = host_pack(arch, sd_np, 20)
    assert stream.shape[0] % 192 == 0 and stream.shape[0] >= len(frags) and bias.shape[0] == len(tiles)
    assert not stream[len(frags):].any()
    want = decode(frags, {k: np.asarray(v, np.float64).astype(np.float32) for k, v in tensors.items()})
    views = np.array([f[0] == "FOLD" and f[1] == "acc" for f in frags])
    assert np.array_equal(stream[:len(frags)][~views], want[~views])            # untouched layers and the view-encoding columns
    got, ref = stream[:len(frags)][views], want[views]
    if integer:
        assert np.array_equal(got, ref)
    else:
        step = np.abs(ref) * 2.0 ** -7 + 1e-30                                  # one bf16 step at that magnitude, at most
        assert (np.abs(got - ref) <= step).all() and (got != ref).mean() < 0.02, float((got != ref).mean())
        assert np.abs(got).max() > 0
    for ti, (tname, row0) in enumerate(tiles):
        b = biases[tname]
        want_b = np.array([b[row0 + r] if row0 + r < len(b) else 0.0 for r in range(16)])
        if tname == "FOLD" and not integer:
            assert np.allclose(bias[ti], want_b, rtol=1e-5, atol=1e-6)
        else:
            assert np.array_equal(bias[ti], want_b.astype(np.float32)), (tname, row0)


# ================================================================================================ GPU
@gpu
@pytest.mark.parametrize("name", FOLDED)
def test_folded_kernels_are_exact_on_integer_weights(dev, name):
    """Key 2 = 2: model(pts, viewdirs) under no_grad runs the folded stream, in both shapes of the weight pipeline (key 0 = 0:
    the pipelined kernel, whose view-direction hooks moved to the skip layer; 41: the per-tile kernel), at the awkward
    counts and with one and two tiles for some workgroups (the relocated hooks on a first, a middle and a last tile; the
    ticket deal).  Integer weights (test_integer_weights_fold_exactly): the float64 reference, bit for bit."""
    from nerf_shared_amd import nerf
    m = X.gpu_model(dev, name)
    m.precision = "bf16"
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    batches = []
    for R, S in X.INFER_SIZES:
        sd, pts, vd, g_raw, ref = X.case(name, R, S)
        batches.append(("%dx%d" % (R, S), pts, vd, ref["raw"]))
    for n in (256 * n_cu + 300, 2 * 256 * n_cu + 513):
        batches.append(("%d points" % n,) + X.tiled_case(name, n))
    # key 2 = 2 without the folded copy is an error, not a silent unfolded run
    bare = nerf.NeRF(**X.ARCHS[name])
    bare.load_state_dict(X.weights(name))
    bare = bare.to(dev)
    bare.precision = "bf16"
    with tuning(2, 2), torch.no_grad():
        with pytest.raises(_lib.NerfAmdError, match="stale or was never made"):
            bare(batches[0][1].to(dev), batches[0][2].to(dev))
    try:
        with tuning(2, 2):
            for variant in (0, 41):
                _lib.check(lib.nerf_amd_set_tuning(0, variant), "set_tuning")
                for what, pts, vd, want in batches:
                    m._model_handle(dev, BF16_FOLDED)
                    with torch.no_grad():
                        raw = m(pts.to(dev), vd.to(dev))
                    torch.cuda.synchronize()
                    X.assert_exact("%s %s folded, variant %d: raw" % (name, what, variant), raw, want)
    finally:
        lib.nerf_amd_set_tuning(0, 0)


def net64_rgb_sigma(arch, sd, pts, vd):
    A = X._arch(arch)
    sd64 = {k: v.double() for k, v in sd.items()}
    flat = pts.double().reshape(-1, 3)
    e_dirs = O.embed(vd.double()[:, None].expand(pts.shape).reshape(-1, 3), A.multires_views, A.i_embed)
    with torch.no_grad():
        return X.net64(sd64, arch, O.embed(flat, A.multires, A.i_embed), e_dirs).reshape(list(pts.shape[:-1]) + [4])


@gpu
@pytest.mark.parametrize("seed,scale", [(0, 1.0), (1, 3.0)])
def test_sigma_is_untouched_and_rgb_is_no_worse(dev, seed, scale):
    """Random weights, 4097 points in [-3, 3]^3 with unit view directions, key 2 = 1 (unfolded) against key 2 = 2 (folded):
    the sigma column is bit-equal (trunk and alpha_linear are the same fragments), and the rgb columns' relative L2 against
    the float64 network is at most 1.25 x the unfolded kernel's, measured here (a CPU rounding model of both gave ratios of
    0.88 - 1.02; the margin is for summation order, which that model does not have)."""
    rng = np.random.default_rng(40 + seed)
    pts = torch.from_numpy(rng.uniform(-3, 3, size=(4097, 1, 3)).astype(np.float32))
    vd = torch.nn.functional.normalize(torch.from_numpy(rng.normal(size=(4097, 3)).astype(np.float32)), dim=-1)
    sd = synth.torch_state_dict(seed, scale, **{**VD, "skips": (4,)})
    ref = net64_rgb_sigma(VD, sd, pts, vd)
    m = P.gpu_model(dev, seed, scale, "bf16", **VD)
    m._model_handle(dev, BF16_FOLDED)
    legs = {}
    for key, leg in ((1, "unfolded"), (2, "folded")):
        with tuning(2, key), torch.no_grad():
            legs[leg] = m(pts.to(dev), vd.to(dev)).cpu()
    torch.cuda.synchronize()
    assert torch.equal(legs["unfolded"][..., 3], legs["folded"][..., 3])
    e_unf, e_fold = X.rel_l2(legs["unfolded"][..., :3], ref[..., :3]), X.rel_l2(legs["folded"][..., :3], ref[..., :3])
    mutual = X.rel_l2(legs["folded"][..., :3], legs["unfolded"][..., :3])
    print("seed %d x%g: rgb relative L2 against float64: unfolded %.3e, folded %.3e (ratio %.3f); folded against unfolded %.3e"
          % (seed, scale, e_unf, e_fold, e_fold / e_unf, mutual))
    assert mutual > 0, "the two legs ran the same kernel"
    assert e_fold <= 1.25 * e_unf, (e_fold, e_unf)


def psnr(a, b):
    mse = float((a.double() - b.double()).square().mean())
    return float("inf") if mse == 0 else -10.0 * np.log10(mse)


def ray_batch(dev, n=300):
    _, _, utils = P.amd()
    K = synth.lego_intrinsics(400, 400)
    return utils.make_ray_batch(400, 400, K, synth.LEGO_C2W, 2.0, 6.0, True, False, device=dev, pix0=70000, n=n)


def render(r, batch, c, f):
    with torch.no_grad():
        out = {k: v.clone() for k, v in r.render_rays(batch, c, f, retraw=True, retweights=True).items()}
    torch.cuda.synchronize()
    return out


UNMOVED = ("z_vals", "weights", "acc_map", "disp_map")


@gpu
def test_render_path_moves_only_rgb(dev):
    """render_rays, 64 + 128 samples, perturb 0, 300 rays, bf16 models (seeds 1 / 19, x3), default (key 2 = 0: folded)
    against key 2 = 1: z_vals, weights, acc_map, disp_map and sigma are bit-equal -- the fine samples come from the coarse
    pass's sigma, which the fold does not touch -- and rgb_map moves by less than the bf16 mode's own distance from the fp32
    kernel on the same rays (PSNR between the legs above the PSNR of the unfolded bf16 render against fp32).  model(pts,
    viewdirs) at the default still runs the unfolded stream: bit-equal to the training forward, folded copy present."""
    _, render_utils, _ = P.amd()
    r = render_utils.Renderer(**P.BASE)
    c, f = P.gpu_model(dev, 1, 3.0, "bf16", **VD), P.gpu_model(dev, 19, 3.0, "bf16", **VD)
    batch = ray_batch(dev)
    fold = render(r, batch, c, f)
    with tuning(2, 1):
        unfold = render(r, batch, c, f)
    for k in UNMOVED:
        assert torch.equal(torch.nan_to_num(fold[k]), torch.nan_to_num(unfold[k])), k
    assert torch.equal(fold["raw"][..., 3], unfold["raw"][..., 3])
    assert not torch.equal(fold["raw"][..., :3], unfold["raw"][..., :3]), "the default render did not run the folded stream"
    c.precision = f.precision = "fp32"
    exact = render(r, batch, c, f)
    c.precision = f.precision = "bf16"
    between, mode = psnr(fold["rgb_map"], unfold["rgb_map"]), psnr(unfold["rgb_map"], exact["rgb_map"])
    print("rgb_map PSNR: folded against unfolded %.2f dB; unfolded bf16 against the fp32 kernel %.2f dB; folded bf16 against fp32 %.2f dB"
          % (between, mode, psnr(fold["rgb_map"], exact["rgb_map"])))
    assert between > mode, (between, mode)
    # model(pts, viewdirs): unfolded at the default, whatever copies exist
    pts = batch[:, None, 0:3] + batch[:, None, 3:6] * fold["z_vals"][..., None]
    vd = batch[:, 8:11].contiguous()
    assert f._packed_copies & _lib.COPY_BF16_FOLD
    with torch.no_grad():
        inferred = f(pts, vd)
    f.requires_grad_(True)
    trained = f(pts, vd)
    f.requires_grad_(False)
    assert trained.requires_grad and torch.equal(inferred, trained.detach())
    with tuning(2, 1), torch.no_grad():
        assert torch.equal(f(pts, vd), inferred)


@gpu
@pytest.mark.parametrize("change", ["adam_step", "load_state_dict", "captured_replays"])
def test_no_stale_fold(dev, change):
    """Render, change the weights (one optim.Adam step; a load_state_dict; two replays of utils.CapturedTrainStep, which
    update the parameters on the device behind autograd's version counters and pack only the training copies), render
    again: the second render differs from the first and equals, bit for bit, the render of fresh models holding the new
    weights -- the folded copy is re-made with every other copy."""
    from nerf_shared_amd import nerf, optim, utils
    _, render_utils, _ = P.amd()
    r = render_utils.Renderer(**dict(P.BASE, N_samples=32, N_importance=32))
    arch = {**VD, "skips": (4,)}

    def make(sds):
        ms = []
        for sd in sds:
            m = nerf.NeRF(**VD)
            m.load_state_dict(sd)
            m.precision = "bf16"
            ms.append(m.to(dev))
        return ms

    c, f = make([synth.torch_state_dict(s, 3.0, **arch) for s in (1, 19)])
    batch = ray_batch(dev, 257)
    before = render(r, batch, c, f)
    assert c._packed_copies & _lib.COPY_BF16_FOLD and f._packed_copies & _lib.COPY_BF16_FOLD
    if change == "adam_step":
        params = list(c.parameters()) + list(f.parameters())
        opt = optim.Adam(params, lr=1e-2, betas=(0.9, 0.999))
        g = torch.Generator(device="cpu").manual_seed(5)
        for p in params:
            p.grad = torch.randn(p.shape, generator=g).to(dev)
        opt.step()
    elif change == "captured_replays":
        K, N, rng = synth.lego_intrinsics(400, 400), 256, np.random.default_rng(8)
        opt = optim.Adam(list(c.parameters()) + list(f.parameters()), lr=1e-3, betas=(0.9, 0.999))
        step = utils.CapturedTrainStep(r, 400, 400, K, 32768, c, f, opt, N)
        for _ in range(2):
            ro, rd = synth.rays_np(400, 400, K, synth.LEGO_C2W, rng.choice(160000, size=N, replace=False))
            step(torch.from_numpy(np.stack([ro, rd], 0)).to(dev), torch.from_numpy(rng.uniform(0, 1, size=(N, 3)).astype(np.float32)).to(dev))
    else:
        for m, s in ((c, 2), (f, 7)):
            m.load_state_dict({k: v.to(dev) for k, v in synth.torch_state_dict(s, 3.0, **arch).items()})
    after = render(r, batch, c, f)
    fresh = render(r, batch, *make([{k: v.detach().clone() for k, v in m.state_dict().items()} for m in (c, f)]))
    assert not torch.equal(after["raw"], before["raw"]), "degenerate test: the render did not change"
    for k in after:
        assert torch.equal(torch.nan_to_num(after[k]), torch.nan_to_num(fresh[k])), k
    with tuning(2, 1):                                      # ... and it was the folded stream that followed the weights
        unfolded = render(r, batch, c, f)
    assert torch.equal(unfolded["raw"][..., 3], after["raw"][..., 3]) and not torch.equal(unfolded["raw"], after["raw"])
