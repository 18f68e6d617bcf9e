"""The live-stretch coarse sampler on the device (nerf_amd_occupancy_coarse_z of csrc/occupancy.hip;
OccupancyGrid.coarse_depths, occupancy.LiveSampler, Renderer.coarse_sampler).

  1. the kernel against tests/live_sampler_mirror.py, bit for bit: z and live_count, over the cases of
     tests/test_live_sampler_host.py (which shows on the CPU that they hold misses, all-live, single- and multi-stretch rays);
  2. an all-live grid leaves render_rays as it was, in every key;
  3. every render path takes its coarse depths from the sampler: the z_vals a path returns are the mirror's, and the paths
     that return none (render_batch) equal, bit for bit, the per-chunk render_rays calls whose z_vals were just checked;
  4. the hook is the hand-made call: nerf_amd_render_rays with io.z_coarse = OccupancyGrid.coarse_depths(...);
  5. train mode with a TrainCull and rays that require grad;  6. captured steps contain it and follow a grid changed in place;
  7. lindisp is refused before any draw or launch.
The shapes are tests/test_train_cull_host.py's: 70 rays of the 400 x 400 lego view, 6 + 5 samples, a 4^3 grid over
[-1.8, 1.8]^3 with a random half-live mask.  A NaN depth (a ray with a NaN near) equals a NaN depth: the payload of a NaN
an addition makes differs between the host and the device, the place of the NaN does not."""
import ctypes
import os

import numpy as np
import pytest
import torch

os.environ.setdefault("NERF_AMD_QUIET", "1")

import live_sampler_mirror as S  # noqa: E402
import test_gpu_parity as P  # noqa: E402
import test_live_sampler_host as LH  # noqa: E402
import test_train_cull_host as H  # noqa: E402
from nerf_shared_amd import _lib, occupancy, render_utils, synth, utils  # noqa: E402
from test_gpu_occupancy import grid_of  # noqa: E402
from test_gpu_train_cull import loss_of, models_of, renderer, reordering_gate, same_bits  # noqa: E402

gpu = pytest.mark.gpu
lib = _lib.lib
R, NC, NI, LO, HI, RES = H.R, H.NC, H.NI, H.LO, H.HI, H.RES
FILL_BITS = 0x7FC12345              # a NaN no result carries
FILL_COUNT = -7
PROBES, PAD = 64, 1                 # of the renderer tests: 64 probes of [2, 6] across a box of four cells a side


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


def t_vals_of(Nc, dev):
    """The ladder the renderer hands the kernels (torch.linspace on the device), on the device and as numpy."""
    t = render_utils._linspace01(Nc, dev)
    return t, t.cpu().numpy()


def assert_depths_equal(got, exp, what=""):
    """Bit for bit; a NaN where the mirror has a NaN."""
    got, exp = np.asarray(got, np.float32), np.asarray(exp, np.float32)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    nan = np.isnan(exp)
    assert np.array_equal(np.isnan(got), nan), what
    g, e = np.where(nan, np.float32(0), got).view(np.uint32), np.where(nan, np.float32(0), exp).view(np.uint32)
    assert np.array_equal(g, e), (what, np.argwhere(g != e)[:5])


# ================================================================================================ 1. the kernel
def run_kernel(dev, grid, rays, t_vals, t_rand, P_, pad, want_count=True):
    """The entry point on numpy rays -> (z, live_count) as numpy; both buffers have one row more than the batch, pre-filled
    with a pattern that no result equals -- the spare row must keep it."""
    Rn, ch = rays.shape
    Nc = t_vals.shape[0]
    rt = torch.from_numpy(np.ascontiguousarray(rays)).to(dev)
    tr = None if t_rand is None else torch.from_numpy(np.ascontiguousarray(t_rand)).to(dev)
    z = torch.tensor(FILL_BITS, dtype=torch.int32, device=dev).expand(Rn + 1, Nc).contiguous()
    count = torch.full((Rn + 1,), FILL_COUNT, dtype=torch.int32, device=dev) if want_count else None
    g = grid._c()
    _lib.check(lib.nerf_amd_occupancy_coarse_z(ctypes.byref(g), rt.data_ptr() if Rn else None, ch, t_vals.data_ptr(), _lib.ptr(tr), Rn, Nc,
                                               P_, pad, 0, int(tr is not None), z.data_ptr(), _lib.ptr(count), _lib.stream_of(dev)),
               "occupancy_coarse_z")
    torch.cuda.synchronize()
    z = z.cpu().numpy()
    assert (z[Rn] == FILL_BITS).all()                                   # nothing written past the batch
    if count is not None:
        count = count.cpu().numpy()
        assert count[Rn] == FILL_COUNT
        count = count[:Rn]
    return z[:Rn].view(np.float32), count


@gpu
@pytest.mark.parametrize("which,outside,ray_ch,Rn,P_,pad,Nc,perturb", LH.KERNEL_CASES)
def test_kernel_equals_the_mirror(dev, which, outside, ray_ch, Rn, P_, pad, Nc, perturb):
    rays, mask, res = LH.kernel_inputs(which, ray_ch)
    rays = rays[:Rn]
    grid = grid_of(dev, LO, HI, res, mask, outside)
    t_dev, t_np = t_vals_of(Nc, dev)
    t_rand = np.random.default_rng(Rn + Nc).random((Rn, Nc), dtype=np.float32) if perturb else None
    with np.errstate(invalid="ignore", over="ignore"):
        exp_z, exp_L, _, _ = S.coarse_depths(rays, mask, LO, HI, outside == "live", P_, pad, t_np, t_rand)
    z, L = run_kernel(dev, grid, rays, t_dev, t_rand, P_, pad)
    assert L.dtype == np.int32 and np.array_equal(L, exp_L), np.argwhere(L != exp_L)[:5]
    assert_depths_equal(z, exp_z, (which, outside, P_, pad, Nc))
    if Rn >= 6:                                                         # the edge rows do what they are there for
        whole = P_ if outside == "live" else 0
        assert exp_L[0] == whole and exp_L[1] == P_ and exp_L[4] == whole and exp_L[5] == whole
        assert np.isnan(exp_z[5]).all() and not np.isnan(exp_z[:4]).any()
        assert (np.diff(exp_z[3]) <= 0).all() and exp_z[3, 0] <= 6.0                    # far < near: the row runs backwards
        warped = (exp_L > 0) & (exp_L < P_)                             # (how many there are: tests/test_live_sampler_host.py)
        if warped.any():
            assert not np.array_equal(exp_z[warped], S.ladder(rays[warped], t_np, None if t_rand is None else t_rand[warped]))
    z2, none = run_kernel(dev, grid, rays, t_dev, t_rand, P_, pad, want_count=False)    # live_count is optional
    assert none is None and np.array_equal(z2.view(np.uint32), z.view(np.uint32))


@gpu
def test_no_rays_and_the_public_call(dev):
    mask = H.half_live_mask()
    grid = grid_of(dev, LO, HI, RES, mask, "empty")
    t_dev, t_np = t_vals_of(7, dev)
    z, L = run_kernel(dev, grid, H.batch_np(8)[:0], t_dev, None, 64, 1)
    assert z.shape == (0, 7) and L.shape == (0,)
    rays = H.batch_np(11)
    t_rand = torch.rand(R, 7, device=dev)
    for tr in (None, t_rand):
        z, L = grid.coarse_depths(torch.from_numpy(rays).to(dev), t_dev, 128, 2, t_rand=tr)
        assert z.dtype == torch.float32 and L.dtype == torch.int32 and not z.requires_grad and z.shape == (R, 7) and L.shape == (R,)
        exp_z, exp_L, _, _ = S.coarse_depths(rays, mask, LO, HI, False, 128, 2, t_np, None if tr is None else tr.cpu().numpy())
        assert np.array_equal(L.cpu().numpy(), exp_L)
        assert_depths_equal(z.cpu().numpy(), exp_z)
    with pytest.raises(ValueError, match="probes"):
        grid.coarse_depths(torch.from_numpy(rays).to(dev), t_dev, 96, 1)
    with pytest.raises(_lib.NerfAmdError):
        grid.coarse_depths(torch.from_numpy(rays).to(dev), t_dev, 64, 1, t_rand=t_rand[:, :3])
    with pytest.raises(_lib.NerfAmdError):
        grid.coarse_depths(torch.from_numpy(rays), t_dev, 64, 1)


# ================================================================================================ 2. all live = no sampler
@gpu
@pytest.mark.parametrize("perturb", [0.0, 1.0])
@pytest.mark.parametrize("ray_ch", [8, 11])
@pytest.mark.parametrize("precision", ["bf16", "fp32_split"])
def test_all_live_grid_leaves_render_rays_as_it_was(dev, precision, ray_ch, perturb):
    mc, mf = models_of(dev, ray_ch, precision, train=False)
    batch = torch.from_numpy(H.batch_np(ray_ch)).to(dev)
    r = renderer(perturb=perturb, use_viewdirs=ray_ch == 11)
    grid = occupancy.OccupancyGrid([LO, HI], RES, outside="live", device=dev)
    with torch.no_grad():
        torch.manual_seed(5)
        plain = r.render_rays(batch, mc, mf, retraw=True, retweights=True)
        r.coarse_sampler = occupancy.LiveSampler(grid, 128, 1)
        torch.manual_seed(5)
        got = r.render_rays(batch, mc, mf, retraw=True, retweights=True)
    assert list(got) == list(plain) and len(plain) == 10
    for k in plain:
        assert same_bits(got[k], plain[k]), k
    assert bool((grid.coarse_depths(batch, render_utils._linspace01(NC, dev), 128, 1)[1] == 128).all())


# ================================================================================================ 3. every path asks the sampler
def mirror_depths(batch_np, t_np, t_rand, outside="empty", mask=None):
    mask = H.half_live_mask() if mask is None else mask
    return S.coarse_depths(batch_np, mask, LO, HI, outside == "live", PROBES, PAD, t_np, t_rand)


@gpu
@pytest.mark.parametrize("perturb", [0.0, 1.0])
def test_every_path_returns_the_mirrors_depths_without_importance_samples(dev, perturb):
    """N_importance = 0, retweights: the z_vals of render_rays -- no-grad, with Renderer.occupancy set, in train mode -- are the
    mirror's as bits.  render_batch returns no z_vals: over three chunks, with pipeline_batch on, and off with
    fuse_chunk_launches on and off, its raw and maps equal those of the per-chunk render_rays calls (same seed)."""
    ray_ch = 11
    batch_np = H.batch_np(ray_ch)
    batch = torch.from_numpy(batch_np).to(dev)
    grid = grid_of(dev, LO, HI, RES, H.half_live_mask(), "empty")
    _, t_np = t_vals_of(NC, dev)
    r = renderer(perturb=perturb, N_importance=0)
    r.coarse_sampler = occupancy.LiveSampler(grid, PROBES, PAD)
    plain = renderer(perturb=perturb, N_importance=0)

    def draws(seed, rows=R):
        torch.manual_seed(seed)
        t_rand = torch.rand([rows, NC], device=dev).cpu().numpy() if perturb > 0 else None
        torch.manual_seed(seed)
        return t_rand

    exp_z, exp_L, _, _ = mirror_depths(batch_np, t_np, draws(3))
    assert ((exp_L > 0) & (exp_L < PROBES)).sum() >= 35                 # most rays are warped
    mc, mf = models_of(dev, ray_ch, "bf16", train=False)
    with torch.no_grad():
        draws(3)
        got = r.render_rays(batch, mc, mf, retraw=True, retweights=True)
        draws(3)
        ref = plain.render_rays(batch, mc, mf, retraw=True, retweights=True)
    assert_depths_equal(got["z_vals"].cpu().numpy(), exp_z, "render_rays")
    assert not same_bits(got["z_vals"], ref["z_vals"]) and not same_bits(got["rgb_map"], ref["rgb_map"])
    r.occupancy = grid
    with torch.no_grad():
        draws(3)
        culled = r.render_rays(batch, mc, mf, retraw=True, retweights=True)
    r.occupancy = None
    assert_depths_equal(culled["z_vals"].cpu().numpy(), exp_z, "render_rays, culled")
    assert 0 < r.last_cull["coarse_live"] < r.last_cull["coarse_total"] == R * NC
    # train mode
    tc, tf = models_of(dev, ray_ch, "bf16")
    draws(3)
    trained = r.render_rays(batch, tc, tf, retraw=True, retweights=True)
    assert trained["rgb_map"].requires_grad and not trained["z_vals"].requires_grad
    assert_depths_equal(trained["z_vals"].detach().cpu().numpy(), exp_z, "render_rays, train mode")
    # render_batch, three chunks
    chunk = 32
    with torch.no_grad():
        draws(4)
        parts = [r.render_rays(batch[i:i + chunk], mc, mf, retraw=True, retweights=True) for i in range(0, R, chunk)]
    t_rand = draws(4, rows=chunk)
    for n, i in enumerate(range(0, R, chunk)):                          # (the chunks' draws follow one another in the generator)
        rows = min(chunk, R - i)
        if perturb > 0:
            torch.manual_seed(4)
            for k in range(n + 1):
                t_rand = torch.rand([min(chunk, R - k * chunk), NC], device=dev).cpu().numpy()
        assert_depths_equal(parts[n]["z_vals"].cpu().numpy(), mirror_depths(batch_np[i:i + rows], t_np, t_rand)[0], "chunk %d" % n)
    for pipeline, fuse in ((True, True), (False, True), (False, False)):
        r.pipeline_batch, r.fuse_chunk_launches = pipeline, fuse
        with torch.no_grad():
            draws(4)
            out = r.render_batch(mc, mf, batch, chunk, True)
        for k in ("raw", "rgb_map", "disp_map", "acc_map"):
            assert same_bits(out[k], torch.cat([p[k] for p in parts], 0)), (pipeline, fuse, k)
    r.pipeline_batch = r.fuse_chunk_launches = True
    with torch.no_grad():
        draws(4)
        dense = plain.render_batch(mc, mf, batch, chunk, True)
    assert not same_bits(out["raw"], dense["raw"])


@gpu
@pytest.mark.parametrize("perturb", [0.0, 1.0])
def test_every_mirror_coarse_depth_occurs_in_the_returned_depths_with_importance_samples(dev, perturb):
    batch_np = H.batch_np(11)
    batch = torch.from_numpy(batch_np).to(dev)
    grid = grid_of(dev, LO, HI, RES, H.half_live_mask(), "empty")
    r = renderer(perturb=perturb)
    r.coarse_sampler = occupancy.LiveSampler(grid, PROBES, PAD)
    mc, mf = models_of(dev, 11, "bf16", train=False)
    torch.manual_seed(6)
    t_rand = torch.rand([R, NC], device=dev).cpu().numpy() if perturb > 0 else None
    exp_z = mirror_depths(batch_np, t_vals_of(NC, dev)[1], t_rand)[0]
    with torch.no_grad():
        torch.manual_seed(6)
        z = r.render_rays(batch, mc, mf, retweights=True)["z_vals"].cpu().numpy()
    assert z.shape == (R, NC + NI)
    zb, eb = z.view(np.uint32), exp_z.view(np.uint32)
    for row in range(R):
        left = list(zb[row])
        for v in eb[row]:
            assert v in left, (row, v)
            left.remove(v)                                              # (a depth that occurs twice is there twice)


# ================================================================================================ 4. the hook = the hand-made call
@gpu
@pytest.mark.parametrize("ray_ch", [8, 11])
def test_render_rays_with_the_hook_is_the_library_call_fed_the_depths_by_hand(dev, ray_ch):
    grid = grid_of(dev, LO, HI, RES, H.half_live_mask(), "empty")
    mc, mf = models_of(dev, ray_ch, "bf16", train=False)
    rays = torch.from_numpy(H.batch_np(ray_ch)).to(dev)
    a, b = renderer(perturb=1.0, use_viewdirs=ray_ch == 11), renderer(perturb=1.0, use_viewdirs=ray_ch == 11)
    a.coarse_sampler = occupancy.LiveSampler(grid, PROBES, PAD)
    with torch.no_grad():
        torch.manual_seed(9)
        got = a.render_rays(rays, mc, mf, retraw=True, retweights=True)
        torch.manual_seed(9)
        plain = b.render_rays(rays, mc, mf, retraw=True, retweights=True)
        # by hand: the draws of one render_rays call (Renderer._draws makes them in the reference's order), the depths from
        # the public OccupancyGrid.coarse_depths on the jitter draws, and the library's render_rays on io.z_coarse
        torch.manual_seed(9)
        hc, hf, cfg, out_ch = b._handles(dev, mc, mf)
        outs = b._alloc_outputs(R, dev, out_ch, True, True)
        z_hand = torch.empty(R, NC, device=dev)
        draws = b._draws(R, dev)
        ws = render_utils._workspace(dev, lib.nerf_amd_render_rays_workspace(cfg, R, out_ch))
        io = b._io(rays, draws, outs, z_hand, ws)
        t_rand = draws.t_rand
        assert t_rand.shape == (R, NC) and io.z_coarse == z_hand.data_ptr()
        z, L = grid.coarse_depths(rays, render_utils._linspace01(NC, dev), PROBES, PAD, t_rand=t_rand)
        z_hand.copy_(z)
        _lib.check(lib.nerf_amd_render_rays(cfg, hc, hf, io, R, _lib.stream_of(dev)), "nerf_amd_render_rays")
        torch.cuda.synchronize()
    assert int(((L > 0) & (L < PROBES)).sum()) >= 35
    assert set(got) == set(outs)
    for k in outs:
        assert same_bits(got[k], outs[k]), k
    assert not same_bits(got["z_vals"], plain["z_vals"]) and not same_bits(got["rgb_map"], plain["rgb_map"])
    with pytest.raises(_lib.NerfAmdError):
        a.render_rays(rays.cpu(), mc, mf)


# ================================================================================================ 5. train mode, culled, ray gradients
@gpu
@pytest.mark.parametrize("precision", ["bf16", "fp32_split"])
def test_train_mode_with_a_train_cull_and_rays_that_require_grad(dev, precision):
    """The depths are constants of the step: columns 6, 7 of the ray gradient are the +0.0 the culled path gives them whatever
    the sampler does, and every gradient is that of the same call fed the same depths by hand (OccupancyGrid.coarse_depths in
    the place of Renderer._coarse_z), under the gate for fp32 sums taken in another order."""
    grid = grid_of(dev, LO, HI, RES, H.half_live_mask(), "empty")
    mc, mf = models_of(dev, 11, precision)
    batch = torch.from_numpy(H.batch_np(11)).to(dev)
    target = torch.from_numpy(np.random.default_rng(2).uniform(0, 1, (R, 3)).astype(np.float32)).to(dev)
    a, b = renderer(perturb=1.0), renderer(perturb=1.0)
    a.train_occupancy, b.train_occupancy = occupancy.TrainCull(grid), occupancy.TrainCull(grid)
    a.coarse_sampler = occupancy.LiveSampler(grid, PROBES, PAD)

    def by_hand(rays, t_rand, z_out):
        z_out.copy_(grid.coarse_depths(rays, render_utils._linspace01(NC, dev), PROBES, PAD, t_rand=t_rand)[0])
    b._coarse_z = by_hand
    params = [p for m in (mc, mf) for p in m.parameters()]

    def run(rend):
        for m in (mc, mf):
            m.zero_grad()
        rays = batch.clone().requires_grad_(True)
        torch.manual_seed(8)
        out = rend.render_rays(rays, mc, mf, retraw=True, retweights=True)
        loss_of(out, target).backward()
        return {k: v.detach() for k, v in out.items()}, rays.grad, [None if p.grad is None else p.grad.clone() for p in params]

    got, g_rays, g_params = run(a)
    ref, e_rays, e_params = run(b)
    del b._coarse_z
    dense, _, _ = run(b)
    for k in ref:
        assert same_bits(got[k], ref[k]), k
    assert not same_bits(got["z_vals"], dense["z_vals"])                # the sampler decides something here
    sa = a.train_occupancy.stats()
    assert 0 < sa["coarse"]["live"] <= sa["coarse"]["total"] == R * NC and sa["fine"]["total"] == R * (NC + NI)
    assert g_rays.shape == (R, 11) and bool(torch.isfinite(g_rays).all()) and g_rays[:, 0:6].abs().max() > 0
    assert not g_rays[:, 6:8].any() and not torch.signbit(g_rays[:, 6:8]).any()         # exactly +0.0
    cols = [0, 1, 2, 3, 4, 5, 8, 9, 10]
    reordering_gate(g_rays[:, cols], e_rays[:, cols])
    assert sum(g is not None for g in g_params) >= 2 * 2 * 9
    for g, e in zip(g_params, e_params):
        assert (g is None) == (e is None)
        if g is not None:
            assert bool(torch.isfinite(g).all())
            reordering_gate(g, e)


# ================================================================================================ 6. captured steps
@gpu
def test_captured_train_step_samples_and_follows_a_grid_changed_in_place(dev):
    """utils.CapturedTrainStep (70 rays, 6 + 5, fp32_split) with coarse_sampler, after
    test_captured_train_step_clips_and_follows_a_grid_changed_in_place: three replays give the losses of three eager steps from
    the same state (rtol 2e-5: the backward's float atomics move the last bits); then set_mask replaces the grid's bits in
    place and the next replay equals an eager step on the new grid, not one on the old grid."""
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
    r.coarse_sampler = occupancy.LiveSampler(grid, PROBES, PAD)

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
def test_captured_pose_step_samples_and_follows_a_grid_changed_in_place(dev):
    """utils.CapturedPoseStep (frozen models, 64 pixels of a 20 x 20 image) with coarse_sampler: three replays against three
    eager steps from the same state, then a fourth after set_mask against an eager step on the new grid, under the same gate."""
    from nerf_shared_amd import optim
    import test_gpu_pose_step as PS
    Hh = W = 20
    K = synth.lego_intrinsics(Hh, W)
    n, steps = 64, 3
    r = renderer()
    mc, mf = PS.frozen_pair(dev, P.VD, "fp32_split", 1.0, seeds=(0, 10))
    with torch.no_grad():
        for m in (mc, mf):
            m.alpha_linear.bias += 1.0
    mc.requires_grad_(False)
    mf.requires_grad_(False)
    pose = torch.from_numpy(PS.lego44()).to(dev)
    with torch.no_grad():
        image = r.render_from_pose(Hh, W, K, 32768, pose[:3], mc, mf, retraw=False)[0]
    rng = np.random.default_rng(12)
    batches = []
    for _ in range(steps + 1):
        idx = rng.choice(Hh * W, size=n, replace=False)
        pix = torch.from_numpy(np.stack([idx % W, idx // W], -1)).to(dev)
        batches.append((pix, image[pix[:, 1], pix[:, 0]].contiguous()))
    mask_a = torch.from_numpy(H.half_live_mask()).to(dev)
    mask_b = ~mask_a
    grid = grid_of(dev, LO, HI, RES, H.half_live_mask(), "empty")
    ptr = grid.words.data_ptr()
    r.coarse_sampler = occupancy.LiveSampler(grid, PROBES, PAD)

    def fresh():
        cam = utils.CameraTransf()
        with torch.no_grad():
            for p, p0 in zip(cam.parameters(), [torch.tensor(PS.TWIST["w"]), torch.tensor(PS.TWIST["v"]), torch.tensor(PS.TWIST["theta"])]):
                p.copy_(p0)
        cam = cam.to(dev)
        return cam, optim.Adam(cam.parameters(), lr=0.01, betas=(0.9, 0.999))

    def eager_run(last_mask):
        grid.set_mask(mask_a)
        cam, opt = fresh()
        losses = []
        for i, (pix, tgt) in enumerate(batches):
            if i == steps:
                grid.set_mask(last_mask)
            opt.zero_grad()
            ro, rd = utils.get_rays_at(Hh, W, K, cam(pose), pix)
            rgb = r.render_from_rays(Hh, W, K, 32768, torch.stack([ro, rd], 0), mc, mf, retraw=True)[0]
            loss = utils.img2mse(rgb, tgt)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        assert all(p.grad is not None and p.grad.abs().max() > 0 for p in cam.parameters())
        return losses

    old, new = eager_run(mask_a), eager_run(mask_b)
    ls, r.coarse_sampler = r.coarse_sampler, None
    unsampled = eager_run(mask_a)
    r.coarse_sampler = ls
    assert abs(unsampled[0] - new[0]) > 1e-3 * abs(new[0])              # the sampler decides something here
    assert abs(old[steps] - new[steps]) > 1e-3 * abs(new[steps])        # ... and so does the grid
    grid.set_mask(mask_a)
    cam2, opt2 = fresh()
    step = utils.CapturedPoseStep(r, Hh, W, K, 32768, mc, mf, cam2, pose, opt2, n)
    got = [float(step(*b)) for b in batches[:steps]]
    grid.set_mask(mask_b)
    assert grid.words.data_ptr() == ptr
    got.append(float(step(*batches[steps])))
    print("eager, new grid", ["%.6e" % v for v in new])
    print("captured       ", ["%.6e" % v for v in got])
    np.testing.assert_allclose(got, new, rtol=2e-5)
    assert all(p.grad is None for m in (mc, mf) for p in m.parameters())


# ================================================================================================ 7. lindisp
@gpu
def test_lindisp_with_a_sampler_is_refused_before_any_draw_or_launch(dev):
    grid = grid_of(dev, LO, HI, RES, H.half_live_mask(), "empty")
    mc, mf = models_of(dev, 11, "bf16", train=False)
    batch = torch.from_numpy(H.batch_np(11)).to(dev)
    r = renderer(perturb=1.0, lindisp=True)
    r.coarse_sampler = occupancy.LiveSampler(grid, PROBES, PAD)
    tc, tf = models_of(dev, 11, "bf16")
    torch.manual_seed(1)
    state = torch.cuda.get_rng_state(dev)
    with torch.no_grad():
        with pytest.raises(_lib.NerfAmdError, match="lindisp"):
            r.render_rays(batch, mc, mf)
        with pytest.raises(_lib.NerfAmdError, match="lindisp"):
            r.render_batch(mc, mf, batch, 32, False)
        r.occupancy = grid
        with pytest.raises(_lib.NerfAmdError, match="lindisp"):
            r.render_rays(batch, mc, mf)
        r.occupancy = None
    with pytest.raises(_lib.NerfAmdError, match="lindisp"):
        r.render_rays(batch, tc, tf)
    assert torch.equal(torch.cuda.get_rng_state(dev), state)            # nothing was drawn
    g = grid._c()
    t = render_utils._linspace01(NC, dev)
    z = torch.empty(R, NC, device=dev)
    assert lib.nerf_amd_occupancy_coarse_z(ctypes.byref(g), batch.data_ptr(), 11, t.data_ptr(), None, R, NC, 64, 1, 1, 0, z.data_ptr(),
                                           None, _lib.stream_of(dev)) == -1
    r.lindisp = False                                                   # the same renderer without lindisp renders
    with torch.no_grad():
        assert bool(torch.isfinite(r.render_rays(batch, mc, mf)["rgb_map"]).all())
