"""The folded bf16 render kernels leave out the colour branch (views_linears.0, rgb_linear) of 16-sample blocks in which no
sample has density (csrc/mlp_bf16_s16.hip view_branch_fold, nerf_amd_set_tuning key 3).

raw2outputs gives a sample with sigma <= 0 the weight 1 - exp(-0) = 0 exactly, so its colour reaches every map as + 0.  A
render that hands out no `raw` and adds no sigma noise therefore need not compute that colour; the kernel decides per
16-point column tile of a wave (all 16 sigmas <= 0, a NaN counts as density, points past the end count as empty), stores
rgb = 0 for such a tile, and runs half of the view branch's MFMAs where one of a wave's two tiles is empty.  What must hold:
  * every map of render_rays is bit-identical with the skip on (key 3 = 0, the default) and off (key 3 = 1);
  * sigma never moves; the rgb of a computed block is the off leg's bit for bit; the rgb of a skipped block is +0.0 -- written,
    not inherited from whatever the workspace held;
  * the skip is off where rgb can matter: raw handed to the caller, sigma noise;
  * the pipelined kernel and the per-tile kernel (key 0 = 41) agree bit for bit with the skip on.
The tests call nerf_amd_render_rays with a workspace of their own (laid out as capi.hip rays_ws_bytes states it: coarse z /
raw / weights, then fine z / raw, each aligned to 256 bytes) and read both passes' raw back from it, so "skipped" and
"computed" are observed per block and not inferred from the maps.
"""
import os

import numpy as np
import pytest
import torch

os.environ.setdefault("NERF_AMD_QUIET", "1")

import test_gpu_parity as P  # noqa: E402
from nerf_shared_amd import _lib, synth  # noqa: E402

gpu = pytest.mark.gpu
lib = _lib.lib
VD = P.VD
VD_15_6 = dict(VD, multires=15, multires_views=6)
MAPS = ("rgb_map", "disp_map", "acc_map", "rgb0", "disp0", "acc0", "z_std")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class tuning:
    """nerf_amd_set_tuning(key, value) for a with-block; back to the default afterwards."""

    def __init__(self, key, value):
        self.key, self.value = key, value

    def __enter__(self):
        _lib.check(lib.nerf_amd_set_tuning(self.key, self.value), "set_tuning")

    def __exit__(self, *exc):
        lib.nerf_amd_set_tuning(self.key, 0)


def test_tuning_key_3_takes_0_and_1():
    assert lib.nerf_amd_set_tuning(3, 1) == 0 and lib.nerf_amd_set_tuning(3, 0) == 0
    assert lib.nerf_amd_set_tuning(3, 2) == -1 and lib.nerf_amd_set_tuning(3, -1) == -1


# ---------------------------------------------------------------------------------------------- models
_MODELS = {}


def model(dev, kind, seed, arch=VD):
    """An 8x256 view-branch bf16 model from synth.torch_state_dict (sharpened x3, the bench check's set); kind:
    mixed   as drawn: sigma changes sign along rays
    empty   alpha_linear.bias = -1e3: no sample has density
    dense   alpha_linear.bias = +1e3: every sample has
    zero+ / zero-   alpha_linear weight and bias +0.0 / -0.0: sigma is a zero everywhere
    nan     alpha_linear.bias = NaN
    hot     dense, rgb_linear.weight scaled by 1e38 and its bias +inf: every rgb is inf or NaN"""
    key = (kind, seed, arch["multires"])
    if key not in _MODELS:
        from nerf_shared_amd import nerf
        sd = synth.torch_state_dict(seed, 3.0, **{**arch, "skips": tuple(arch["skips"])})
        w, b = sd["alpha_linear.weight"], sd["alpha_linear.bias"]
        if kind == "empty":
            b.fill_(-1e3)
        elif kind in ("dense", "hot"):
            b.fill_(1e3)
        elif kind in ("zero+", "zero-"):
            w.fill_(0.0 if kind == "zero+" else -0.0)
            b.fill_(0.0 if kind == "zero+" else -0.0)
        elif kind == "nan":
            b.fill_(float("nan"))
        else:
            assert kind == "mixed"
        if kind == "hot":
            sd["rgb_linear.weight"].mul_(1e38)
            sd["rgb_linear.bias"].fill_(float("inf"))
        m = nerf.NeRF(**arch)
        m.load_state_dict(sd)
        m.precision = "bf16"
        _MODELS[key] = m.to(dev).requires_grad_(False)
    return _MODELS[key]


def pair(dev, kind, arch=VD):
    return model(dev, kind, 1, arch), model(dev, kind, 19, arch)


def renderer(**over):
    _, render_utils, _ = P.amd()
    return render_utils.Renderer(**dict(P.BASE, **over))


def rays(dev, n):
    _, _, utils = P.amd()
    K = synth.lego_intrinsics(400, 400)
    return utils.make_ray_batch(400, 400, K, synth.LEGO_C2W, 2.0, 6.0, True, False, device=dev, pix0=70000, n=n)


# ---------------------------------------------------------------------------------------------- one render, raw observed
def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def render(r, batch, c, f, ws=None, seed=None):
    """nerf_amd_render_rays as Renderer.render_rays(batch, c, f) calls it (no raw, no weights asked for), but into the
    workspace `ws` (made here if None).  Returns (maps, [raw of the coarse pass, raw of the fine pass], ws); the raws are
    copies of what the field kernels left in the workspace, [R, S, 4]."""
    dev, R = batch.device, batch.shape[0]
    Nc, Ni = int(r.N_samples), int(r.N_importance)
    if seed is not None:
        torch.manual_seed(seed)
    hc, hf, cfg, och = r._handles(dev, c, f)
    draws, z_pre = r._chunk_inputs(batch, False)
    need = lib.nerf_amd_render_rays_workspace(cfg, R, och)
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    assert ws.numel() >= need
    outs = r._alloc_outputs(R, dev, och, False, False)
    io = r._io(batch, draws, outs, z_pre, ws)
    assert not io.raw and (r.raw_noise_std > 0) == bool(io.noise0)
    with torch.cuda.device(dev):
        _lib.check(lib.nerf_amd_render_rays(cfg, hc, hf, io, R, _lib.stream_of(dev)), "nerf_amd_render_rays")
    torch.cuda.synchronize()
    al = lambda n: (n + 255) & ~255
    off, raws = 0, []
    for S, what in ((Nc, "zrw"), (Nc + Ni, "zr")) if Ni else ((Nc, "zrw"),):
        for part in what:
            n = R * S * 4 * (och if part == "r" else 1)
            if part == "r":
                raws.append(ws[off:off + n].view(torch.float32).view(R, S, och).clone())
            off += al(n)
    assert off == need
    return outs, raws, ws


def dead_points(raw):
    """[P] bool: the point lies in a 16-point block (points 16b .. 16b+15 of the pass, in launch order) whose sigmas are all <= 0."""
    sigma = raw[..., 3].reshape(-1)
    n = sigma.numel()
    pad = torch.ones(-n % 16, dtype=torch.bool, device=raw.device)
    blocks = torch.cat([sigma <= 0, pad]).view(-1, 16).all(1)
    return blocks.repeat_interleave(16)[:n], blocks


def wave_patterns(blocks):
    """The (first block empty, second block empty) pairs that occur among the 32-point waves of a pass."""
    b = torch.cat([blocks, torch.ones(blocks.numel() % 2, dtype=torch.bool, device=blocks.device)]).view(-1, 2)
    return {(bool(x), bool(y)) for x, y in torch.unique(b, dim=0).tolist()}


def check(on, off, skipping=True):
    """Maps bit-equal; sigma bit-equal; rgb of every block the off leg's, or +0.0 where the block is empty and the skip is on.
    Returns per pass (blocks, empty blocks, wave patterns)."""
    (maps_on, raws_on, _), (maps_off, raws_off, _) = on, off
    for k in MAPS:
        if k in maps_off:
            assert same_bits(maps_on[k], maps_off[k]), k
    assert len(raws_on) == len(raws_off)
    stats = []
    for a, b in zip(raws_on, raws_off):
        assert same_bits(a[..., 3], b[..., 3]), "sigma moved"
        dead, blocks = dead_points(b)
        want = b[..., :3].reshape(-1, 3).clone()
        if skipping:
            want[dead] = 0.0
        assert same_bits(a[..., :3].reshape(-1, 3), want), "rgb is neither the off leg's nor a written zero"
        stats.append((blocks.numel(), int(blocks.sum()), wave_patterns(blocks)))
    return stats


def both_legs(r, batch, c, f, seed=None):
    on = render(r, batch, c, f, seed=seed)
    with tuning(3, 1):
        off = render(r, batch, c, f, seed=seed)
    return on, off


# ---------------------------------------------------------------------------------------------- GPU
@gpu
@pytest.mark.parametrize("R", [1, 5, 33, 257])
@pytest.mark.parametrize("kind", ["empty", "dense", "mixed"])
def test_maps_are_bit_identical(dev, kind, R):
    """64 + 128 samples; R = 1, 5, 33, 257 rays: 64 ... 16448 coarse and 192 ... 49344 fine points, none a multiple of the
    256-point workgroup tile -- the last workgroup of every launch has waves that lie past P altogether (R = 1: six of the
    coarse launch's eight) -- and from one workgroup to 193.  (A wave that is partly past P: test_a_block_spans_two_rays.)"""
    r = renderer()
    c, f = pair(dev, kind)
    stats = check(*both_legs(r, rays(dev, R), c, f))
    print(kind, R, stats)
    for n, empty, _ in stats:
        if kind == "empty":
            assert empty == n
        if kind == "dense":
            assert empty == 0


@gpu
@pytest.mark.parametrize("kind", ["empty", "mixed"])
def test_a_block_spans_two_rays(dev, kind):
    """8 + 8 samples: a 16-point block is two rays of the coarse pass and one of the fine pass; 37 rays: the coarse pass ends
    in half a block (296 points = 18.5 blocks), whose missing points count as empty."""
    r = renderer(N_samples=8, N_importance=8)
    stats = check(*both_legs(r, rays(dev, 37), *pair(dev, kind)))
    print(kind, stats)
    assert stats[0][0] == 19 and stats[1][0] == 37


@gpu
@pytest.mark.parametrize("over", [dict(white_bkgd=False), dict(perturb=1.0), dict(white_bkgd=False, perturb=1.0)],
                         ids=["black", "perturb", "black_perturb"])
def test_other_renders(dev, over):
    """white_bkgd off; perturb 1 with the generator re-seeded in front of each leg."""
    r = renderer(**over)
    stats = check(*both_legs(r, rays(dev, 129), *pair(dev, "mixed"), seed=7))
    assert sum(e for _, e, _ in stats) > 0, stats


@gpu
@pytest.mark.parametrize("kind", ["empty", "dense", "mixed"])
def test_multires_15_6(dev, kind):
    stats = check(*both_legs(renderer(), rays(dev, 33), *pair(dev, kind, VD_15_6)))
    print(kind, stats)
    if kind == "empty":
        assert all(e == n for n, e, _ in stats)


@gpu
def test_block_patterns(dev):
    """The mixed models on 257 rays: among the 32-point waves there are waves with both blocks empty, with both computed, and
    with exactly one empty -- either one (the half-issued view branch).  Asserted from the off leg's sigma, not assumed; check()
    then holds every block of every pattern to its contract."""
    stats = check(*both_legs(renderer(), rays(dev, 257), *pair(dev, "mixed")))
    seen = set().union(*[p for _, _, p in stats])
    print(stats)
    assert seen == {(False, False), (False, True), (True, False), (True, True)}, seen
    assert all(0 < e < n for n, e, _ in stats), stats


@gpu
def test_raw_to_the_caller_is_computed(dev):
    """retraw=True: raw is bit-equal to the off leg's and holds the colour of samples without density -- the skip is off."""
    r = renderer()
    batch = rays(dev, 65)
    for kind in ("empty", "mixed"):
        c, f = pair(dev, kind)
        with torch.no_grad():
            on = {k: v.clone() for k, v in r.render_rays(batch, c, f, retraw=True).items()}
            with tuning(3, 1):
                off = {k: v.clone() for k, v in r.render_rays(batch, c, f, retraw=True).items()}
        for k in off:
            assert same_bits(on[k], off[k]), (kind, k)
        dead, blocks = dead_points(on["raw"])
        assert blocks.any() and bool((on["raw"][..., :3].reshape(-1, 3)[dead] != 0).any()), kind


@gpu
def test_sigma_noise_is_computed(dev):
    """raw_noise_std = 1 (generator re-seeded per leg): sigma + noise has its own sign, so nothing is skipped -- both passes' raw
    and every map equal the off leg's bit for bit."""
    r = renderer(raw_noise_std=1.0)
    stats = check(*both_legs(r, rays(dev, 65), *pair(dev, "mixed"), seed=11), skipping=False)
    assert sum(e for _, e, _ in stats) > 0, stats


@gpu
@pytest.mark.parametrize("kind", ["zero+", "zero-"])
def test_sigma_zero_is_empty(dev, kind):
    """alpha_linear all +0.0 / all -0.0: sigma is a zero everywhere, which is <= 0 whatever its sign: every block is skipped.
    (Measured on MI355X: the matrix pipe returns +0.0 for the -0.0 weights and bias too -- the count of sign bits is printed --
    so the kernel's `<= 0`, an IEEE comparison that takes -0.0 as it takes +0.0, is what covers a negative zero.)"""
    on, off = both_legs(renderer(), rays(dev, 33), *pair(dev, kind))
    for raw in off[1]:
        assert bool((raw[..., 3] == 0).all())
    print(kind, "sign bits of sigma:", [int((bits(raw[..., 3]) < 0).sum()) for raw in off[1]], "of", [raw[..., 3].numel() for raw in off[1]])
    assert all(e == n for n, e, _ in check(on, off))


@gpu
def test_sigma_nan_is_computed(dev):
    """NaN in alpha_linear.bias: `NaN <= 0` is false, the tile is computed, and both legs hold the same NaNs."""
    on, off = both_legs(renderer(), rays(dev, 33), *pair(dev, "nan"))
    assert all(bool(torch.isnan(raw[..., 3]).all()) for raw in off[1])
    assert all(e == 0 for _, e, _ in check(on, off))


@gpu
def test_skipped_rgb_is_written_not_inherited(dev):
    """One workspace, two renders: first the dense models with rgb_linear scaled to overflow (every rgb in the workspace is inf
    or NaN), then the empty models with the skip on.  0 * NaN is NaN: the maps are finite (disp_map is the reference's 0 / 0
    where nothing was hit, in both legs) and equal the off leg's, because the skipped points' rgb is stored as zero."""
    r = renderer()
    batch = rays(dev, 65)
    _, hot, ws = render(r, batch, *pair(dev, "hot"))
    for raw in hot:
        assert not bool(torch.isfinite(raw[..., :3]).any())
    on = render(r, batch, *pair(dev, "empty"), ws=ws)
    assert on[2].data_ptr() == ws.data_ptr()
    for raw in on[1]:
        assert bool((bits(raw[..., :3]) == 0).all())
    with tuning(3, 1):
        _, hot2, _ = render(r, batch, *pair(dev, "hot"), ws=ws)
        off = render(r, batch, *pair(dev, "empty"), ws=ws)
    assert all(e == n for n, e, _ in check(on, off))
    for k in ("rgb_map", "acc_map", "rgb0", "acc0", "z_std"):
        assert bool(torch.isfinite(on[0][k]).all()), k


@gpu
def test_pipelined_equals_per_tile(dev):
    """The pipelined kernel against the per-tile kernel (key 0 = 41), both with the skip on, mixed models, 257 rays: maps and
    both passes' raw bit for bit."""
    r = renderer()
    batch = rays(dev, 257)
    c, f = pair(dev, "mixed")
    pipelined = render(r, batch, c, f)
    with tuning(0, 41):
        per_tile = render(r, batch, c, f)
        with tuning(3, 1):
            per_tile_off = render(r, batch, c, f)
    for k in MAPS:
        assert same_bits(pipelined[0][k], per_tile[0][k]), k
    for a, b in zip(pipelined[1], per_tile[1]):
        assert same_bits(a, b)
    assert sum(e for _, e, _ in check(per_tile, per_tile_off)) > 0
