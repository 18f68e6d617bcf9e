"""GPU tests (-m gpu) of the pixel selection of the pose-estimation workload (demo_est_rel_pose.py:35-47, :75-79) on the device:
interest points, dilation, compaction, the per-step draw (utils.find_POI, utils.PixelSampler), the captured pose step that
draws its own pixels (utils.CapturedPoseStep(sampler=...)) and the whole loop (utils.estimate_relative_pose).

Everything selected is integer arithmetic or a plain load, so every comparison with the numpy mirror
(tests/pixel_select_mirror.py, written from the definitions in include/nerf_amd.h) is EQUALITY; the losses compared are
forward passes from equal states, which are deterministic, and are compared bit for bit as well."""
import os

import numpy as np
import pytest
import torch

os.environ.setdefault("NERF_AMD_QUIET", "1")
pytestmark = pytest.mark.gpu

from nerf_shared_amd import _lib, synth  # noqa: E402
import pixel_select_mirror as mirror  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def checkerboard(H=24, W=31):
    """Squares of 6 pixels, two grey levels, plus seeded noise of 0..15 per channel: uint8 [H, W, 3] with corners to find."""
    y, x = np.mgrid[0:H, 0:W]
    base = (((y // 6) + (x // 6)) % 2) * 180 + 30
    noise = np.random.default_rng(5).integers(0, 16, size=(H, W, 3))
    return (base[..., None] + noise).astype(np.uint8)


def random_image(H, W, seed, C=3):
    return np.random.default_rng(seed).integers(0, 256, size=(H, W, C)).astype(np.uint8)


def ref_float(img_u8):
    """The demo's conversion, demo_est_rel_pose.py:36."""
    return (np.array(img_u8) / 255.).astype(np.float32)


# ------------------------------------------------------------------------------------------------ 1. detector
def gpu_interest_mask(dev, img, quality=1):
    H, W, C = img.shape
    t = torch.from_numpy(img).to(dev).contiguous()
    ws = torch.empty(int(_lib.lib.nerf_amd_interest_points_workspace(H, W)) // 8, dtype=torch.int64, device=dev)
    mask = torch.full((H, W), 77, dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib.nerf_amd_interest_points(t.data_ptr(), H, W, C, quality, ws.data_ptr(), mask.data_ptr(), _lib.stream_of(dev)),
               "nerf_amd_interest_points")
    return mask.cpu().numpy()


DETECTOR_IMAGES = {
    "checkerboard_24x31": checkerboard(),
    "random_70x67": random_image(70, 67, 1),
    "random_2x5": random_image(2, 5, 2),
    "random_1x1": random_image(1, 1, 3),
    "flat_9x11": np.full((9, 11, 3), 128, np.uint8),
    "random_70x67_rgba": random_image(70, 67, 4, C=4),
}


@pytest.mark.parametrize("name", list(DETECTOR_IMAGES))
def test_interest_points_equal_the_mirror(dev, name):
    from nerf_shared_amd import utils
    img = DETECTOR_IMAGES[name]
    want = mirror.interest_mask(img, 1)
    got = gpu_interest_mask(dev, img)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    if img.shape[0] * img.shape[1] > 100:
        for q in (50, 100):
            assert np.array_equal(gpu_interest_mask(dev, img, q), mirror.interest_mask(img, q)), q
    pts = utils.find_POI(img)
    assert pts.is_cuda and pts.dtype == torch.int32 and tuple(pts.shape) == (int(want.sum()), 2)
    assert np.array_equal(pts.cpu().numpy(), mirror.compact(want))                   # row-major order
    if name.startswith("flat"):
        assert want.sum() == 0 and tuple(pts.shape) == (0, 2)
    if name in ("checkerboard_24x31", "random_70x67"):
        assert 0 < want.sum() < want.size // 4, "degenerate test: the detector found nothing, or everything"
    if name == "checkerboard_24x31":                                                 # a float image is quantised with to8b first
        as_float = ref_float(img) * np.float32(0.999)
        want_f = mirror.compact(mirror.interest_mask(utils.to8b(as_float), 1))
        assert np.array_equal(utils.find_POI(as_float).cpu().numpy(), want_f) and want_f.shape[0] > 0


# ------------------------------------------------------------------------------------------------ 2. dilation
def corner_mask():
    m = np.zeros((9, 13), np.uint8)
    m[0, 0] = m[0, 12] = m[8, 0] = m[8, 12] = m[4, 6] = 1
    return m


def sparse_mask(H, W, fraction, seed):
    return (np.random.default_rng(seed).random((H, W)) < fraction).astype(np.uint8)


def gpu_dilate(dev, m, k, I):
    t = torch.from_numpy(m).to(dev)
    out = torch.full_like(t, 77)
    _lib.check(_lib.lib.nerf_amd_dilate_mask(t.data_ptr(), m.shape[0], m.shape[1], k, I, out.data_ptr(), _lib.stream_of(dev)),
               "nerf_amd_dilate_mask")
    return out.cpu().numpy()


@pytest.mark.parametrize("I", [1, 3])
@pytest.mark.parametrize("k", [1, 3, 4, 5])
def test_dilation_equals_successive_iterations(dev, k, I):
    for m in (corner_mask(), sparse_mask(70, 67, 0.01, 8)):
        assert np.array_equal(gpu_dilate(dev, m, k, I), mirror.dilate(m, k, I)), m.shape
    grey = (sparse_mask(9, 13, 0.2, 9) * np.random.default_rng(10).integers(1, 256, size=(9, 13))).astype(np.uint8)
    assert np.array_equal(gpu_dilate(dev, grey, k, I), mirror.dilate(grey, k, I))           # a maximum, not an OR


# ------------------------------------------------------------------------------------------------ 3. compaction
def last_only(H, W):
    m = np.zeros((H, W), np.uint8)
    m[-1, -1] = 1
    return m


COMPACT_MASKS = {
    "empty_9x13": np.zeros((9, 13), np.uint8),
    "full_9x13": np.ones((9, 13), np.uint8),
    "full_16x16_one_block": np.full((16, 16), 255, np.uint8),
    "last_pixel_70x67": last_only(70, 67),
    "30_percent_70x67": sparse_mask(70, 67, 0.3, 11),
    "50_percent_130x129": sparse_mask(130, 129, 0.5, 12),
    "50_percent_300x301_runs_of_two": sparse_mask(300, 301, 0.5, 13),           # 353 blocks: the scan's threads own two counts each
}


@pytest.mark.parametrize("name", list(COMPACT_MASKS))
def test_compaction_is_coords_of_mask_in_row_major_order(dev, name):
    m = COMPACT_MASKS[name]
    H, W = m.shape
    t = torch.from_numpy(m).to(dev)
    blocks = torch.empty((H * W + 255) // 256, dtype=torch.int32, device=dev)
    out = torch.full((H * W, 2), -7, dtype=torch.int32, device=dev)
    count = torch.full((), -1, dtype=torch.int64, device=dev)
    _lib.check(_lib.lib.nerf_amd_compact_mask(t.data_ptr(), H, W, blocks.data_ptr(), out.data_ptr(), count.data_ptr(),
                                              _lib.stream_of(dev)), "nerf_amd_compact_mask")
    want = mirror.compact(m)
    M = int(count)
    assert M == want.shape[0] == int((m != 0).sum())
    assert np.array_equal(out[:M].cpu().numpy(), want)
    assert bool((out[M:] == -7).all())                          # nothing written past the count
    if name == "50_percent_130x129":
        assert M > 8000


# ------------------------------------------------------------------------------------------------ 4. the draw
SAMPLER_IMAGE = random_image(70, 67, 21)


def points_of(M, seed=31):
    """M distinct pixels of the 70 x 67 image as (x, y), shuffled, with a few repeated (the sampler de-duplicates)."""
    rng = np.random.default_rng(seed + M)
    idx = rng.choice(70 * 67, size=M, replace=False)
    pts = np.stack([idx % 67, idx // 67], -1)
    return np.concatenate([pts, pts[:3]], 0)


def check_draws(sampler, image_f32, M, n, seed, counters, W, region):
    for c in counters:
        pix, tgt = sampler.draw()
        want = mirror.draw_pixels(M, n, seed, c, W=W, region=region)
        got = pix.cpu().numpy()
        assert pix.dtype == torch.int32 and got.shape == (n, 2) and np.array_equal(got, want), c
        assert len({tuple(p) for p in got.tolist()}) == n
        assert np.array_equal(tgt.cpu().numpy(), image_f32[want[:, 1], want[:, 0], :3]), c


@pytest.mark.parametrize("M,n", [(1, 1), (5, 5), (37, 16), (1000, 64), (4097, 512)])
def test_draws_from_a_region_equal_the_mirror(dev, M, n):
    from nerf_shared_amd import utils
    pts = points_of(M)
    s = utils.PixelSampler(SAMPLER_IMAGE, n, strategy="interest_point", points=pts, seed=1234, device=dev)
    mask = np.zeros((70, 67), np.uint8)
    mask[pts[:, 1], pts[:, 0]] = 1
    region = mirror.compact(mask)
    assert s.M == M == region.shape[0] and np.array_equal(s.region.cpu().numpy(), region)
    img = ref_float(SAMPLER_IMAGE)
    assert np.array_equal(s.image.cpu().numpy(), img)
    p0, t0 = s.pixels, s.target
    check_draws(s, img, M, n, 1234, range(5), 67, region)
    assert int(s.draw_count) == 5
    assert s.draw()[0] is p0 and s.draw()[1] is t0                  # fixed buffers
    s.reset(2 ** 32 - 2)
    check_draws(s, img, M, n, 1234, [2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32], 67, region)
    assert int(s.draw_count) == 2 ** 32 + 1
    assert np.array_equal(s.pixels.cpu().numpy(), mirror.draw_pixels(M, n, 1234, 0, region=region))     # low 32 bits: draw 0 again


def test_random_draws_over_a_whole_400x400_image(dev):
    from nerf_shared_amd import utils
    img8 = random_image(400, 400, 22)
    s = utils.PixelSampler(torch.from_numpy(img8), 512, strategy="random", seed=9, device=dev)
    assert s.M == 160000 and s.region is None
    check_draws(s, ref_float(img8), 160000, 512, 9, range(5), 400, None)
    assert int(s.draw_count) == 5


def test_dilated_region_of_the_builtin_detector(dev):
    from nerf_shared_amd import utils
    img = checkerboard()
    s = utils.PixelSampler(img, 32, strategy="interest_region", kernel_size=4, dil_iter=2, seed=2, device=dev)
    region = mirror.region_of(img, "interest_region", kernel_size=4, dil_iter=2)
    assert np.array_equal(s.region.cpu().numpy(), region) and s.M == region.shape[0]
    check_draws(s, ref_float(img), s.M, 32, 2, range(3), 31, region)
    p = utils.PixelSampler(img, 4, strategy="interest_point", seed=2, device=dev)
    assert np.array_equal(p.region.cpu().numpy(), mirror.region_of(img, "interest_point"))


def test_four_channels_and_a_row_strided_view_gather_correctly(dev):
    from nerf_shared_amd import utils
    H, W = 20, 23
    rng = np.random.default_rng(40)
    wide = torch.from_numpy(rng.random((H, W + 5, 4)).astype(np.float32)).to(dev)
    view = wide[:, 2:2 + W, :]                                       # row stride (W + 5) * 4, four channels, offset start
    s = utils.PixelSampler(view, 64, strategy="random", seed=5)
    assert s.image.data_ptr() == view.data_ptr()                     # used in place
    host = view.cpu().numpy()
    check_draws(s, host, H * W, 64, 5, range(3), W, None)
    rgba8 = random_image(H, W, 41, C=4)
    s8 = utils.PixelSampler(rgba8, 64, strategy="random", seed=5, device=dev)
    check_draws(s8, ref_float(rgba8), H * W, 64, 5, range(3), W, None)
    with torch.no_grad():
        view.mul_(0.5)                                               # an image used in place can be rewritten between draws
    check_draws(s, view.cpu().numpy(), H * W, 64, 5, [3], W, None)


# ------------------------------------------------------------------------------------------------ 5. capture
def test_a_captured_draw_advances_on_the_device(dev):
    from nerf_shared_amd import utils
    pts = points_of(1000)
    s = utils.PixelSampler(SAMPLER_IMAGE, 64, strategy="interest_point", points=pts, seed=77, device=dev)
    region = s.region.cpu().numpy()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        s.draw()
    torch.cuda.current_stream(dev).wait_stream(side)
    s.reset(0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pix, tgt = s.draw()
    got = []
    for _ in range(5):
        graph.replay()
        got.append((pix.clone(), tgt.clone()))
    img = ref_float(SAMPLER_IMAGE)
    for c, (p, t) in enumerate(got):
        want = mirror.draw_pixels(1000, 64, 77, c, region=region)
        assert np.array_equal(p.cpu().numpy(), want), c
        assert np.array_equal(t.cpu().numpy(), img[want[:, 1], want[:, 0]]), c
    assert int(s.draw_count) == 5


# ------------------------------------------------------------------------------------------------ 6. the captured pose step
VD = dict(D=8, W=256, output_ch=5, skips=[4], use_viewdirs=True, multires=10, multires_views=4)
RENDER = dict(perturb=0.0, N_importance=32, N_samples=32, use_viewdirs=True, white_bkgd=True, raw_noise_std=0.0, ndc=False,
              lindisp=False, near=2.0, far=6.0)
TWIST = dict(w=[0.30, -0.25, 0.35], v=[0.30, -0.20, 0.25], theta=0.2)
_SCENES = {}


def lego44():
    return np.concatenate([synth.LEGO_C2W, np.array([[0, 0, 0, 1]], np.float32)], 0)


def scene(dev, precision):
    """The fogged synthetic fields of the captured-pose-step tests (smooth weights, density bias + 1), frozen, a renderer with
    32 + 32 samples and the 20 x 20 view from LEGO_C2W; built once per precision."""
    if precision not in _SCENES:
        from nerf_shared_amd import nerf, render_utils
        models = []
        for seed in (0, 10):
            m = nerf.NeRF(**VD)
            m.load_state_dict(synth.torch_state_dict(seed, 1.0, **{**VD, "skips": tuple(VD["skips"])}))
            with torch.no_grad():
                m.alpha_linear.bias += 1.0
            m = m.to(dev).requires_grad_(False)
            m.precision = precision
            models.append(m)
        r = render_utils.Renderer(**RENDER)
        pose = torch.from_numpy(lego44()).to(dev)
        with torch.no_grad():
            image = r.render_from_pose(20, 20, synth.lego_intrinsics(20, 20), 32768, pose[:3], models[0], models[1], retraw=False)[0]
        _SCENES[precision] = (r, models[0], models[1], pose, image.contiguous())
    return _SCENES[precision]


def twisted_cam(dev):
    from nerf_shared_amd import optim, utils
    cam = utils.CameraTransf()
    with torch.no_grad():
        cam.w.copy_(torch.tensor(TWIST["w"])); cam.v.copy_(torch.tensor(TWIST["v"])); cam.theta.copy_(torch.tensor(TWIST["theta"]))
    cam = cam.to(dev)
    return cam, optim.Adam(cam.parameters(), lr=0.01, betas=(0.9, 0.999))


@pytest.mark.parametrize("precision", ["fp32_split", "bf16"])
def test_captured_pose_step_draws_its_own_pixels(dev, precision):
    from nerf_shared_amd import utils
    H = W = 20
    n = 64
    K = synth.lego_intrinsics(H, W)
    r, mc, mf, pose, image = scene(dev, precision)
    assert float(image.std()) > 1e-3, "degenerate test: a featureless target"
    img_host = image.cpu().numpy()
    cam, opt = twisted_cam(dev)
    before = [p.detach().clone() for p in cam.parameters()]
    sampler = utils.PixelSampler(image, n, strategy="random", seed=3)
    step = utils.CapturedPoseStep(r, H, W, K, 32768, mc, mf, cam, pose, opt, n, sampler=sampler)
    assert all(torch.equal(p, b) for p, b in zip(cam.parameters(), before))
    assert opt._together[0]["step"] == 0 and int(opt._device_scalars[0][0]) == 0
    assert all(not st["exp_avg"].any() and not st["exp_avg_sq"].any() for st in opt.state.values())
    assert int(sampler.draw_count) == 0
    assert step.pixels is sampler.pixels and step.target is sampler.target

    cam2, opt2 = twisted_cam(dev)
    plain = utils.CapturedPoseStep(r, H, W, K, 32768, mc, mf, cam2, pose, opt2, n)
    pix0 = mirror.draw_pixels(H * W, n, 3, 0, W=W)
    tgt0 = torch.from_numpy(img_host[pix0[:, 1], pix0[:, 0]]).to(dev)
    loss_plain = plain(torch.from_numpy(pix0).to(dev), tgt0).clone()
    loss = step().clone()
    assert np.array_equal(step.pixels.cpu().numpy(), pix0)
    print("%s: first loss with sampler %.9e, fed the same pixels %.9e" % (precision, float(loss), float(loss_plain)))
    assert float(loss) > 1e-7 and torch.equal(loss, loss_plain)                # the forward is deterministic
    for _ in range(5):
        step()
    pix5 = mirror.draw_pixels(H * W, n, 3, 5, W=W)
    assert np.array_equal(step.pixels.cpu().numpy(), pix5)
    assert np.array_equal(step.target.cpu().numpy(), img_host[pix5[:, 1], pix5[:, 0]])
    assert int(sampler.draw_count) == 6
    assert opt._together[0]["step"] == 6 == int(opt.state_dict()["state"][0]["step"]) and int(opt._device_scalars[0][0]) == 6
    assert not all(torch.equal(p, b) for p, b in zip(cam.parameters(), before)), "degenerate test: the replays did not move the pose"

    with pytest.raises(_lib.NerfAmdError, match="without arguments"):
        step(torch.from_numpy(pix0).to(dev), tgt0)
    with pytest.raises(_lib.NerfAmdError, match="needs both"):
        plain()
    cam3, opt3 = twisted_cam(dev)
    with pytest.raises(_lib.NerfAmdError, match="sampler draws"):
        utils.CapturedPoseStep(r, H, W, K, 32768, mc, mf, cam3, pose, opt3, 32, sampler=sampler)


# ------------------------------------------------------------------------------------------------ 7. the whole loop
def test_estimate_relative_pose(dev):
    from nerf_shared_amd import optim, utils
    H = W = 20
    K = synth.lego_intrinsics(H, W)
    r, mc, mf, pose, image = scene(dev, "fp32_split")
    with torch.no_grad():
        start = twisted_cam(dev)[0](pose).detach().clone()              # the target pose moved by the known twist
    torch.manual_seed(11)
    res = utils.estimate_relative_pose(mc, mf, r, image, start, K, 32768, steps=6, batch_size=64, strategy="random", seed=3)
    got_pose, losses = res
    assert got_pose.is_cuda and tuple(got_pose.shape) == (4, 4) and losses.is_cuda and tuple(losses.shape) == (6,)
    assert bool(torch.isfinite(losses).all()) and float(losses.min()) > 0
    step = res.step
    assert int(step.sampler.draw_count) == 6 and step.optimizer._together[0]["step"] == 6
    with torch.no_grad():
        assert torch.equal(got_pose, step.cam_transf(start))
    assert step.optimizer.param_groups[0]["lr"] == 0.01 * 0.8 ** (6 / 100)

    torch.manual_seed(11)                                               # the same initial seven numbers, fed draw 0 by hand
    cam = utils.CameraTransf().to(dev)
    opt = optim.Adam(cam.parameters(), lr=0.01, betas=(0.9, 0.999))
    plain = utils.CapturedPoseStep(r, H, W, K, 32768, mc, mf, cam, start, opt, 64)
    pix0 = mirror.draw_pixels(H * W, 64, 3, 0, W=W)
    tgt0 = image[torch.from_numpy(pix0[:, 1]).long().to(dev), torch.from_numpy(pix0[:, 0]).long().to(dev)].contiguous()
    first = plain(torch.from_numpy(pix0).to(dev), tgt0)
    print("first loss: estimate_relative_pose %.9e, by hand %.9e" % (float(losses[0]), float(first)))
    assert torch.equal(losses[0], first)

    mf.requires_grad_(True)
    try:
        with pytest.raises(_lib.NerfAmdError, match="requires_grad_"):
            utils.estimate_relative_pose(mc, mf, r, image, start, K, 32768, steps=1, batch_size=64, strategy="random")
    finally:
        mf.requires_grad_(False)


def test_estimate_relative_pose_draws_inside_the_interest_region(dev):
    from nerf_shared_amd import utils
    img = checkerboard()                                                # 24 x 31: H != W
    H, W = img.shape[:2]
    r, mc, mf, pose, _ = scene(dev, "bf16")
    res = utils.estimate_relative_pose(mc, mf, r, img, pose, synth.lego_intrinsics(H, W), 32768, steps=3, batch_size=32,
                                       strategy="interest_region", kernel_size=3, dil_iter=1, seed=4)
    region = mirror.region_of(img, "interest_region", kernel_size=3, dil_iter=1)
    assert 32 <= region.shape[0] < H * W
    sampler = res.step.sampler
    assert (sampler.H, sampler.W) == (24, 31) and np.array_equal(sampler.region.cpu().numpy(), region)
    drawn = res.step.pixels.cpu().numpy()
    inside = {tuple(p) for p in region.tolist()}
    assert all(tuple(p) in inside for p in drawn.tolist())
    assert np.array_equal(drawn, mirror.draw_pixels(region.shape[0], 32, 4, 2, region=region))
    assert bool(torch.isfinite(res.losses).all())


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_on_the_device_path(dev):
    from nerf_shared_amd import utils
    img = checkerboard()
    M = mirror.region_of(img, "interest_point").shape[0]
    with pytest.raises(_lib.NerfAmdError, match="distinct"):
        utils.PixelSampler(img, M + 1, strategy="interest_point", device=dev)
    with pytest.raises(_lib.NerfAmdError, match="distinct"):
        utils.PixelSampler(img, 24 * 31 + 1, strategy="random", device=dev)
    flat = np.full((9, 11, 3), 128, np.uint8)
    for strategy in ("interest_point", "interest_region"):
        with pytest.raises(_lib.NerfAmdError, match="no interest points"):
            utils.PixelSampler(flat, 1, strategy=strategy, device=dev)
    utils.PixelSampler(flat, 1, strategy="random", device=dev)
    with pytest.raises(_lib.NerfAmdError, match="ROCm"):
        utils.PixelSampler(img, 4, strategy="random", device="cpu")
    r, mc, mf, pose, image = scene(dev, "bf16")
    cam, opt = twisted_cam(dev)
    host_sampler = object()
    with pytest.raises(_lib.NerfAmdError, match="PixelSampler"):
        utils.CapturedPoseStep(r, 20, 20, synth.lego_intrinsics(20, 20), 32768, mc, mf, cam, pose, opt, 64, sampler=host_sampler)
    # the C entry points refuse what would read or write out of bounds
    t = torch.zeros(4, 4, dtype=torch.uint8, device=dev)
    assert _lib.lib.nerf_amd_dilate_mask(t.data_ptr(), 4, 4, 3, 1, t.data_ptr(), _lib.stream_of(dev)) == -1          # in place
    s = utils.PixelSampler(img, 4, strategy="random", device=dev)
    for M_bad, n_bad in ((24 * 31, 24 * 31 + 1), (24 * 31 + 1, 4), (0, 0)):
        assert _lib.lib.nerf_amd_draw_pixels(M_bad, n_bad, 0, s.draw_count.data_ptr(), None, 24, 31, s.image.data_ptr(), 31 * 3, 3,
                                             s.pixels.data_ptr(), s.target.data_ptr(), _lib.stream_of(dev)) == -1
    assert int(s.draw_count) == 0
