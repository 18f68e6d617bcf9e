"""Ray bounds on the device (nerf_amd_occupancy_ray_bounds of csrc/occupancy.hip; OccupancyGrid.ray_bounds,
occupancy.RayBounds, Renderer.ray_bounds).

  1. the kernel against tests/ray_bounds_mirror.py, bit for bit: rays_out, bounds and span, edge rays, partly filled blocks;
  2. an all-live grid is the identity, for the bounds and for render_rays in every key;
  3. the hook is the hand-made call: a renderer with ray_bounds equals a renderer without it that is fed the clipped batch --
     render_rays, render from a pose in chunks, render_batch in train mode in chunks (the clip-once rule), ray gradients;
  4. captured steps contain it and follow a grid changed in place;
  5. convex containment, on the device;  6. it still learns.
The shapes are tests/test_train_cull_host.py's: 70 rays of the 400 x 400 lego view, 6 + 5 samples, a 4^3 grid over
[-1.8, 1.8]^3 with a random half-live mask; tests/test_ray_bounds_host.py shows on the mirror that they narrow most rays and
miss some."""
import ctypes
import os

import numpy as np
import pytest
import torch

os.environ.setdefault("NERF_AMD_QUIET", "1")

import occupancy_mirror as M  # noqa: E402
import ray_bounds_mirror as B  # noqa: E402
import test_gpu_parity as P  # noqa: E402
import test_ray_bounds_host as RH  # noqa: E402
import test_train_cull_host as H  # noqa: E402
from nerf_shared_amd import _lib, occupancy, synth, utils  # noqa: E402
from test_gpu_occupancy import grid_of, random_mask  # noqa: E402
from test_gpu_train_cull import loss_of, models_of, renderer, reordering_gate, same_bits  # noqa: E402

gpu = pytest.mark.gpu
lib = _lib.lib
R, NC, NI, LO, HI, RES = H.R, H.NC, H.NI, H.LO, H.HI, H.RES
FILL_BITS = 0x7FC12345              # a NaN no result carries: copied NaNs are numpy's 0x7FC00000, computed values are finite
FILL_SPAN = -7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


# ================================================================================================ 1. the kernel
def edge_rows(ray_ch, mask, lo, hi):
    """Six rays in front of the batch: one that misses the box, one whose origin (and whole span) lies inside a live cell,
    near == far, far < near, a NaN direction component, a NaN near."""
    base = H.batch_np(11)[[3, 20, 41, 55]].copy()
    n = np.array(mask.shape)
    cell = np.argwhere(mask)[len(np.argwhere(mask)) // 2]
    centre = np.array(lo) + (cell + 0.5) * (np.array(hi) - np.array(lo)) / n
    rows = np.zeros((6, 11), np.float32)
    rows[0] = [5, 5, 5, 0, 0, 1, 2, 6, 0, 0, 1]
    rows[1] = [*centre, 1e-3, 0, 0, 2, 6, 1, 0, 0]
    rows[2:6] = base
    rows[2, 6:8] = 4.0
    rows[3, 6:8] = [6.0, 2.0]
    rows[4, 4] = np.nan
    rows[5, 6] = np.nan
    return np.ascontiguousarray(rows[:, :ray_ch])


def run_kernel(dev, grid, rays, P_, pad, want=(True, True, True)):
    """The entry point on numpy rays -> (rays_out, bounds, span) as numpy (None where not asked for); every output buffer has
    one row more than the batch and is pre-filled with a pattern that no result equals -- the spare row must keep it."""
    Rn, ch = rays.shape
    rt = torch.from_numpy(np.ascontiguousarray(rays)).to(dev)
    fill = torch.tensor(FILL_BITS, dtype=torch.int32, device=dev)
    outs = [fill.expand(Rn + 1, ch).contiguous() if want[0] else None, fill.expand(Rn + 1, 2).contiguous() if want[1] else None,
            torch.full((Rn + 1, 2), FILL_SPAN, dtype=torch.int32, device=dev) if want[2] else None]
    g = grid._c()
    _lib.check(lib.nerf_amd_occupancy_ray_bounds(ctypes.byref(g), rt.data_ptr() if Rn else None, ch, Rn, P_, pad, _lib.ptr(outs[0]),
                                                 _lib.ptr(outs[1]), _lib.ptr(outs[2]), _lib.stream_of(dev)), "ray_bounds")
    torch.cuda.synchronize()
    res = []
    for o, pat in zip(outs, (FILL_BITS, FILL_BITS, FILL_SPAN)):
        if o is None:
            res.append(None)
            continue
        o = o.cpu().numpy()
        assert (o[Rn] == pat).all()                                     # nothing written past the batch
        res.append(o[:Rn])
    return res


def check_kernel(got, exp, Rn):
    for name, g, e in zip(("rays_out", "bounds", "span"), got, exp):
        if g is None:
            continue
        e = e[:Rn]
        e = e.view(np.int32) if e.dtype == np.float32 else e
        assert g.shape == e.shape and np.array_equal(g, e), (name, Rn, np.argwhere(g != e)[:5])


@gpu
@pytest.mark.parametrize("ray_ch", [8, 11])
@pytest.mark.parametrize("outside", ["live", "empty"])
@pytest.mark.parametrize("which", ["half_live_4", "random_8x6x5"])
def test_kernel_equals_the_mirror(dev, which, outside, ray_ch):
    res, mask = (RES, H.half_live_mask()) if which == "half_live_4" else ((8, 6, 5), random_mask((8, 6, 5), 0.3, 4))
    grid = grid_of(dev, LO, HI, res, mask, outside)
    full = np.concatenate([edge_rows(ray_ch, mask, LO, HI), H.batch_np(ray_ch)], 0)                  # 76 rows
    rays = np.resize(full, (257, ray_ch))                              # the rows again and again: rows [0, R) are R's batch
    assert np.array_equal(rays[:76].view(np.uint32), full.view(np.uint32))
    narrowed = missed = 0
    for P_ in (64, 128, 1024):
        for pad in (0, 1, 3):
            exp = B.ray_bounds(rays, mask, LO, HI, outside == "live", P_, pad)
            for Rn in (1, 3, 5, 76, 257):                               # a single wave, partly filled blocks, more than one block
                check_kernel(run_kernel(dev, grid, rays[:Rn], P_, pad), exp, Rn)
            b, span = exp[1][6:76], exp[2][6:76]
            narrowed += int(((b[:, 0] > 2.0) | (b[:, 1] < 6.0)).sum())
            missed += int((span[:, 0] < 0).sum())
    assert narrowed >= 9 * 10
    if outside == "empty" and which == "half_live_4":
        assert missed >= 1                                              # (tests/test_ray_bounds_host.py: at P = 64)
    # the edge rows do what they are there for (P = 64, pad = 1)
    _, b, span = B.ray_bounds(full, mask, LO, HI, outside == "live", 64, 1)
    whole = [0, 63]
    assert list(span[0]) == (whole if outside == "live" else [-1, -1]) and list(span[1]) == whole
    assert list(span[4]) == list(span[5]) == (whole if outside == "live" else [-1, -1])
    assert np.array_equal(b[[0, 1, 4, 5]].view(np.uint32), full[[0, 1, 4, 5], 6:8].view(np.uint32))
    assert span[2, 0] in (-1, 0) and span[2, 1] in (-1, 63) and list(b[2]) == [4.0, 4.0]
    # each output alone, and no rays at all
    exp = B.ray_bounds(rays[:76], mask, LO, HI, outside == "live", 128, 1)
    for i in range(3):
        want = tuple(j == i for j in range(3))
        got = run_kernel(dev, grid, rays[:76], 128, 1, want)
        assert [g is not None for g in got] == list(want)
        check_kernel(got, exp, 76)
    got = run_kernel(dev, grid, rays[:0], 64, 1)
    assert all(g.shape[0] == 0 for g in got)


# ================================================================================================ 2. all live = identity
@gpu
def test_all_live_grid_returns_the_rays_own_bounds(dev):
    grid = occupancy.OccupancyGrid([LO, HI], RES, outside="live", device=dev)
    mask = np.ones(RES, bool)
    rays = np.concatenate([edge_rows(11, mask, LO, HI), H.batch_np(11)], 0)
    for P_, pad in ((64, 0), (256, 1), (4096, 7)):
        bounds, span = grid.ray_bounds(torch.from_numpy(rays).to(dev), P_, pad)
        assert bounds.dtype == torch.float32 and span.dtype == torch.int32 and not bounds.requires_grad
        assert np.array_equal(bounds.cpu().numpy().view(np.uint32), rays[:, 6:8].view(np.uint32))
        assert (span.cpu().numpy() == [0, P_ - 1]).all()


@gpu
@pytest.mark.parametrize("ray_ch", [8, 11])
@pytest.mark.parametrize("precision", ["bf16", "fp32_split"])
def test_all_live_grid_leaves_render_rays_as_it_was(dev, precision, ray_ch):
    mc, mf = models_of(dev, ray_ch, precision, train=False)
    batch = torch.from_numpy(H.batch_np(ray_ch)).to(dev)
    r = renderer(perturb=1.0, use_viewdirs=ray_ch == 11)
    with torch.no_grad():
        torch.manual_seed(5)
        plain = r.render_rays(batch, mc, mf, retraw=True, retweights=True)
        r.ray_bounds = occupancy.RayBounds(occupancy.OccupancyGrid([LO, HI], RES, outside="live", device=dev), 64, 1)
        torch.manual_seed(5)
        got = r.render_rays(batch, mc, mf, retraw=True, retweights=True)
    assert list(got) == list(plain) and len(plain) == 10
    for k in plain:
        assert same_bits(got[k], plain[k]), k


# ================================================================================================ 3. the hook = the hand-made call
PROBES, PAD = 64, 1


def clipped_by_hand(grid, batch):
    """The batch with columns 6, 7 replaced from OccupancyGrid.ray_bounds (autograd reaches the other columns of `batch`)."""
    bounds, span = grid.ray_bounds(batch, PROBES, PAD)
    assert not bounds.requires_grad
    return torch.cat([batch[:, 0:6], bounds, batch[:, 8:]], 1), bounds, span


def pair(dev, **over):
    """(a renderer with ray_bounds on the half-live grid, one without, the grid)."""
    grid = grid_of(dev, LO, HI, RES, H.half_live_mask(), "empty")
    with_rb, without = renderer(**over), renderer(**over)
    with_rb.ray_bounds = occupancy.RayBounds(grid, PROBES, PAD)
    return with_rb, without, grid


@gpu
@pytest.mark.parametrize("ray_ch", [8, 11])
def test_render_rays_with_the_hook_is_render_rays_of_the_clipped_batch(dev, ray_ch):
    a, b, grid = pair(dev, perturb=1.0, use_viewdirs=ray_ch == 11)
    mc, mf = models_of(dev, ray_ch, "bf16", train=False)
    batch = torch.from_numpy(H.batch_np(ray_ch)).to(dev)
    hand, bounds, span = clipped_by_hand(grid, batch)
    both = (bounds[:, 0] > batch[:, 6]) & (bounds[:, 1] < batch[:, 7])
    assert int(both.sum()) >= 35 and int((span[:, 0] < 0).sum()) >= 1         # (tests/test_ray_bounds_host.py, on the mirror)
    with torch.no_grad():
        torch.manual_seed(9)
        got = a.render_rays(batch, mc, mf, retraw=True, retweights=True)
        torch.manual_seed(9)
        ref = b.render_rays(hand, mc, mf, retraw=True, retweights=True)
        torch.manual_seed(9)
        plain = b.render_rays(batch, mc, mf, retraw=True, retweights=True)
    assert list(got) == list(ref)
    for k in ref:
        assert same_bits(got[k], ref[k]), k
    assert not same_bits(got["z_vals"], plain["z_vals"]) and not same_bits(got["rgb_map"], plain["rgb_map"])
    z = got["z_vals"]
    assert bool((z >= bounds[:, :1]).all()) and bool((z <= bounds[:, 1:]).all())       # every sample inside the clipped span
    # sigma noise is allowed (nothing is resurrected), and a batch on another device than the grid is refused
    a.raw_noise_std = b.raw_noise_std = 1.0
    with torch.no_grad():
        torch.manual_seed(9)
        got = a.render_rays(batch, mc, mf)
        torch.manual_seed(9)
        ref = b.render_rays(hand, mc, mf)
    assert same_bits(got["rgb_map"], ref["rgb_map"])
    with pytest.raises(_lib.NerfAmdError):
        a.render_rays(batch.cpu(), mc, mf)
    with pytest.raises(_lib.NerfAmdError):
        a.ray_bounds.apply(batch.cpu())


@gpu
@pytest.mark.parametrize("culled", [False, True])
def test_render_from_a_pose_in_chunks_clips_once(dev, culled):
    a, b, grid = pair(dev)
    if culled:
        a.occupancy = b.occupancy = grid
    mc, mf = models_of(dev, 11, "bf16", train=False)
    Hh = W = 20
    K = synth.lego_intrinsics(Hh, W)
    c2w = torch.from_numpy(synth.LEGO_C2W)
    batch = utils.make_ray_batch(Hh, W, K, synth.LEGO_C2W, a.near, a.far, True, False, device=dev)
    hand, bounds, span = clipped_by_hand(grid, batch)
    assert int((bounds[:, 1] - bounds[:, 0] < 4.0).sum()) >= 100
    with torch.no_grad():
        rgb, disp, acc, extras = a.render(Hh, W, K, mc, mf, chunk=100, c2w=c2w, retraw=True)
        ref = b.render_batch(mc, mf, hand, 100, True)
        ref_cull = b.last_cull
        twice = b.render_batch(mc, mf, clipped_by_hand(grid, hand)[0], 100, True)
    got = dict(rgb_map=rgb, disp_map=disp, acc_map=acc, **extras)
    assert set(got) == set(ref)
    for k in ref:
        assert same_bits(got[k].reshape(ref[k].shape), ref[k]), k
    assert not same_bits(ref["rgb_map"], twice["rgb_map"])             # clipping is not idempotent: a second clip would show
    if culled:
        assert a.last_cull == ref_cull and 0 < a.last_cull["fine_live"] < a.last_cull["fine_total"]


@gpu
@pytest.mark.parametrize("culled", [False, True])
@pytest.mark.parametrize("precision", ["bf16", "fp32_split"])
def test_render_batch_in_train_mode_in_chunks_clips_once(dev, precision, culled):
    """Outputs and parameter gradients of render_batch over three chunks of a training pair: the train-mode loop renders
    chunk by chunk, and must not clip a chunk that the whole batch's clip has already narrowed."""
    a, b, grid = pair(dev)
    if culled:
        a.train_occupancy, b.train_occupancy = occupancy.TrainCull(grid), occupancy.TrainCull(grid)
    mc, mf = models_of(dev, 11, precision)
    batch = torch.from_numpy(H.batch_np(11)).to(dev)
    target = torch.from_numpy(np.random.default_rng(2).uniform(0, 1, (R, 3)).astype(np.float32)).to(dev)
    hand = clipped_by_hand(grid, batch)[0]
    params = [p for m in (mc, mf) for p in m.parameters()]
    names = [("coarse." if m is mc else "fine.") + n for m in (mc, mf) for n, _ in m.named_parameters()]

    def run(rend, rays):
        for m in (mc, mf):
            m.zero_grad()
        out = rend.render_batch(mc, mf, rays, 32, True)
        assert out["rgb_map"].requires_grad
        loss_of(out, target).backward()
        return {k: v.detach() for k, v in out.items()}, [None if p.grad is None else p.grad.clone() for p in params]

    got, g_got = run(a, batch)
    ref, g_ref = run(b, hand)
    if culled:
        sa, sb = a.train_occupancy.stats(), b.train_occupancy.stats()
        assert sa == sb and 0 < sa["fine"]["live"] < sa["fine"]["total"] == R * (NC + NI) and sa["fine"]["overflow"] == 0
    twice, _ = run(b, clipped_by_hand(grid, hand)[0])
    assert list(got) == list(ref)
    for k in ref:
        assert same_bits(got[k], ref[k]), k
    assert not same_bits(ref["rgb_map"], twice["rgb_map"])             # a second clip would show
    assert sum(g is not None for g in g_ref) >= 2 * 2 * 9
    for name, g, e in zip(names, g_got, g_ref):
        assert (g is None) == (e is None), name
        if g is None:
            continue
        assert g.abs().max() > 0, name
        if "output_linear" in name:         # float atomics accumulate the head of a model without view branch (csrc/backward.hip)
            reordering_gate(g, e)
        else:
            assert same_bits(g, e), (name, float((g - e).abs().max()))


@gpu
@pytest.mark.parametrize("precision", ["bf16", "fp32_split"])
def test_ray_gradients_of_a_frozen_pair_pass_the_clip(dev, precision):
    a, b, grid = pair(dev)
    mc, mf = models_of(dev, 11, precision, train=False)
    batch = torch.from_numpy(H.batch_np(11)).to(dev)
    target = torch.full((R, 3), 0.5, device=dev)
    rays = batch.clone().requires_grad_(True)
    got = a.render_rays(rays, mc, mf)
    assert got["rgb_map"].requires_grad
    loss_of(got, target).backward()
    rays2 = batch.clone().requires_grad_(True)
    ref = b.render_rays(clipped_by_hand(grid, rays2)[0], mc, mf)
    loss_of(ref, target).backward()
    assert same_bits(got["rgb_map"], ref["rgb_map"]) and same_bits(got["rgb0"], ref["rgb0"])
    assert all(p.grad is None for m in (mc, mf) for p in m.parameters())
    g, e = rays.grad, rays2.grad
    assert g.shape == e.shape == (R, 11) and g[:, 0:6].abs().max() > 0 and g[:, 8:11].abs().max() > 0
    cols = [0, 1, 2, 3, 4, 5, 8, 9, 10]
    reordering_gate(g[:, cols], e[:, cols])
    assert not g[:, 6:8].any() and not torch.signbit(g[:, 6:8]).any()                  # exactly +0.0
    # render_batch, the same way
    rays3 = batch.clone().requires_grad_(True)
    out = a.render_batch(mc, mf, rays3, 32, False)
    loss_of(out, target).backward()
    assert same_bits(out["rgb_map"], ref["rgb_map"])
    reordering_gate(rays3.grad[:, cols], e[:, cols])
    assert not rays3.grad[:, 6:8].any() and not torch.signbit(rays3.grad[:, 6:8]).any()


# ================================================================================================ 4. captured steps
@gpu
def test_captured_train_step_clips_and_follows_a_grid_changed_in_place(dev):
    """utils.CapturedTrainStep (70 rays, 6 + 5, fp32_split) with ray_bounds: three replays give the losses of three eager
    steps from the same state (the gate of test_captured_train_step_culls_and_follows_a_refreshed_grid: rtol 2e-5); then
    set_mask replaces the grid's bits in place -- words.data_ptr() unchanged -- and the next replay equals an eager step on
    the new grid, not one on the old grid: the captured kernel reads the grid's words at replay."""
    from nerf_shared_amd import nerf, optim
    arch, precision = P.VD, "fp32_split"
    K = synth.lego_intrinsics(400, 400)
    rng = np.random.default_rng(5)
    N, steps = R, 3
    batches = []
    for _ in range(steps + 1):
        idx = rng.choice(160000, size=N, replace=False)
        ro, rd = synth.rays_np(400, 400, K, synth.LEGO_C2W, idx)
        batches.append((torch.from_numpy(np.stack([ro, rd], 0)).to(dev), torch.from_numpy(rng.uniform(0, 1, size=(N, 3)).astype(np.float32)).to(dev)))

    def fresh():
        ms = []
        for seed in (1, 19):
            m = nerf.NeRF(**arch)
            m.load_state_dict(synth.torch_state_dict(seed, 3.0, **{**arch, "skips": tuple(arch["skips"])}))
            m.precision = precision
            ms.append(m.to(dev))
        return ms, optim.Adam(list(ms[0].parameters()) + list(ms[1].parameters()), lr=5e-4, betas=(0.9, 0.999))

    mask_a = torch.from_numpy(H.half_live_mask()).to(dev)
    mask_b = ~mask_a
    grid = grid_of(dev, LO, HI, RES, H.half_live_mask(), "empty")
    ptr = grid.words.data_ptr()
    r = renderer()
    r.ray_bounds = occupancy.RayBounds(grid, PROBES, PAD)

    def eager_step(ms, opt, i):
        opt.zero_grad()
        rays, tgt = batches[i]
        rgb, _, _, ex = r.render_from_rays(400, 400, K, 32768, rays, ms[0], ms[1], retraw=True)
        loss = utils.img2mse(rgb, tgt) + utils.img2mse(ex["rgb0"], tgt)
        loss.backward()
        opt.step()
        return float(loss.detach())

    def eager_run(last_mask):
        grid.set_mask(mask_a)
        ms, opt = fresh()
        losses = [eager_step(ms, opt, i) for i in range(steps)]
        grid.set_mask(last_mask)
        return losses + [eager_step(ms, opt, steps)]

    old, new = eager_run(mask_a), eager_run(mask_b)
    # (two eager runs from one state: the backward's float atomics move the last bits, hence the gate and not equality)
    np.testing.assert_allclose(old[:steps], new[:steps], rtol=2e-5)
    assert abs(old[steps] - new[steps]) > 1e-3 * abs(new[steps])      # the grids tell the step apart
    grid.set_mask(mask_a)
    assert grid.words.data_ptr() == ptr
    ms2, opt2 = fresh()
    step = utils.CapturedTrainStep(r, 400, 400, K, 32768, ms2[0], ms2[1], opt2, N)
    got = [float(step(*batches[i])) for i in range(steps)]
    grid.set_mask(mask_b)
    assert grid.words.data_ptr() == ptr
    got.append(float(step(*batches[steps])))
    print("eager, new grid", ["%.6f" % v for v in new])
    print("eager, old grid", ["%.6f" % v for v in old])
    print("captured       ", ["%.6f" % v for v in got])
    np.testing.assert_allclose(got, new, rtol=2e-5)
    assert abs(got[steps] - old[steps]) > 1e-3 * abs(old[steps])


@gpu
def test_captured_pose_step_clips(dev):
    """utils.CapturedPoseStep (frozen models, 64 pixels of a 20 x 20 image) with ray_bounds: three replays against three
    eager steps from the same state, under the same gate."""
    from nerf_shared_amd import optim
    import test_gpu_pose_step as S
    Hh = W = 20
    K = synth.lego_intrinsics(Hh, W)
    n, steps = 64, 3
    r = renderer()
    mc, mf = S.frozen_pair(dev, P.VD, "fp32_split", 1.0, seeds=(0, 10))
    with torch.no_grad():
        for m in (mc, mf):
            m.alpha_linear.bias += 1.0
    mc.requires_grad_(False)
    mf.requires_grad_(False)
    pose = torch.from_numpy(S.lego44()).to(dev)
    with torch.no_grad():
        image = r.render_from_pose(Hh, W, K, 32768, pose[:3], mc, mf, retraw=False)[0]
    rng = np.random.default_rng(12)
    batches = []
    for _ in range(steps):
        idx = rng.choice(Hh * W, size=n, replace=False)
        pix = torch.from_numpy(np.stack([idx % W, idx // W], -1)).to(dev)
        batches.append((pix, image[pix[:, 1], pix[:, 0]].contiguous()))
    grid = grid_of(dev, LO, HI, RES, H.half_live_mask(), "empty")
    r.ray_bounds = occupancy.RayBounds(grid, PROBES, PAD)

    def fresh():
        cam = utils.CameraTransf()
        with torch.no_grad():
            for p, p0 in zip(cam.parameters(), [torch.tensor(S.TWIST["w"]), torch.tensor(S.TWIST["v"]), torch.tensor(S.TWIST["theta"])]):
                p.copy_(p0)
        cam = cam.to(dev)
        return cam, optim.Adam(cam.parameters(), lr=0.01, betas=(0.9, 0.999))

    def eager_run():
        cam, opt = fresh()
        losses = []
        for pix, tgt in batches:
            opt.zero_grad()
            ro, rd = utils.get_rays_at(Hh, W, K, cam(pose), pix)
            rgb = r.render_from_rays(Hh, W, K, 32768, torch.stack([ro, rd], 0), mc, mf, retraw=True)[0]
            loss = utils.img2mse(rgb, tgt)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        assert all(p.grad is not None and p.grad.abs().max() > 0 for p in cam.parameters())
        return losses

    eager = eager_run()
    rb, r.ray_bounds = r.ray_bounds, None
    unclipped = eager_run()
    r.ray_bounds = rb
    assert abs(unclipped[0] - eager[0]) > 1e-3 * abs(eager[0])          # the clip decides something here
    cam2, opt2 = fresh()
    step = utils.CapturedPoseStep(r, Hh, W, K, 32768, mc, mf, cam2, pose, opt2, n)
    got = [float(step(*b)) for b in batches]
    print("eager   ", ["%.6e" % v for v in eager])
    print("captured", ["%.6e" % v for v in got])
    np.testing.assert_allclose(got, eager, rtol=2e-5)
    assert all(p.grad is None for m in (mc, mf) for p in m.parameters())


# ================================================================================================ 5. convex containment
@gpu
def test_convex_containment_on_the_device(dev):
    """The 16^3 block of tests/test_ray_bounds_host.py, 512 of its rays, the 192-point ladder: every sample that grid.query
    calls live lies inside the kernel's bounds (pad >= 1)."""
    rays_np, mask, n = RH.convex_case(2)
    rays_np = rays_np[:512]
    grid = grid_of(dev, RH.BOX_LO, RH.BOX_HI, n, mask, "empty")
    rays = torch.from_numpy(rays_np).to(dev)
    z = torch.from_numpy(B.ladder(rays_np, 192)).to(dev)
    pts = rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]
    on = grid.query(pts)
    on_mirror = M.live(M.lookup(M.ray_points(rays_np, z.cpu().numpy()).reshape(-1, 3), RH.BOX_LO, RH.BOX_HI, n), mask, False)
    assert on.shape == z.shape and int(on.sum()) == int(on_mirror.sum()) > 1000          # (116 of the 512 rays meet the block)
    for P_, pad in ((64, 1), (256, 1), (1024, 2)):
        bounds, span = grid.ray_bounds(rays, P_, pad)
        assert bool((bounds[:, 0] >= rays[:, 6]).all()) and bool((bounds[:, 0] <= bounds[:, 1]).all()) and bool((bounds[:, 1] <= rays[:, 7]).all())
        out = on & ((z < bounds[:, :1]) | (z > bounds[:, 1:]))
        narrowed = (span[:, 0] >= 0) & ((bounds[:, 0] > rays[:, 6]) | (bounds[:, 1] < rays[:, 7]))
        assert int(narrowed.sum()) >= 100 and int(out.sum()) == 0, (P_, pad, int(out.sum()))


# ================================================================================================ 6. it still learns
@gpu
def test_it_still_learns_with_ray_bounds(dev):
    """tools/train_demo.py's sphere scene, 600 steps with --occupancy 32 --occupancy-warmup 200 --occupancy-refresh 16
    --ray-bounds 256 against 600 dense steps from the same seed: the test PSNR (rendered with the bounds on) is no lower than
    the dense run's minus the spread of the dense run over three seeds (profiles/occupancy_train.json, the margin of
    test_it_still_learns), and nothing overflows after the calibration.

    Measured: dense 25.037 dB, with ray bounds 24.933 dB, margin 1.010 dB; no overflow.  That is at the pad train_culled trains
    with (32 probe spacings: half a scene unit either side of the span).  At pad 1 and pad 8 the same run ended at 22.608 and
    22.596 dB and this test failed (profiles/occupancy_bounds.json; DESIGN.md section 8e.2 gives what was measured and
    what is only supposed about the cause).  Pad 32 was chosen among {1, 8, 32} on this scene and seed: the test guards
    the demo's schedule, it does not show that 32 is right elsewhere."""
    import json
    import sys
    sys.path.insert(0, os.path.join(P.REPO, "tools"))
    import train_demo
    with open(os.path.join(P.REPO, "profiles", "occupancy_train.json")) as f:
        margin = float(json.load(f)["learning"]["dense_psnr_spread"])
    dense = train_demo.run(steps=600, seed=0, verbose=False)[0]
    clipped, state = train_demo.run(steps=600, seed=0, verbose=False, occupancy_res=32, occupancy_warmup=200, occupancy_refresh=16,
                                    ray_bounds_probes=256)
    stats = clipped["occupancy"]["stats"]
    print("test PSNR after 600 steps: dense %.3f dB, with ray bounds %.3f dB, margin %.3f dB; %s"
          % (dense["psnr_after"], clipped["psnr_after"], margin, stats))
    rb = state[4].ray_bounds
    assert isinstance(rb, occupancy.RayBounds) and (rb.probes, rb.pad) == (256, 32) and state[4].train_occupancy is None
    assert margin > 0 and dense["psnr_after"] > dense["psnr_before"] + 3
    assert clipped["psnr_after"] >= dense["psnr_after"] - margin
    for name in ("coarse", "fine"):
        assert stats[name]["overflow"] == 0 and 0 < stats[name]["live"] < stats[name]["total"]
