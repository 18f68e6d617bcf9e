#!/usr/bin/env python3
"""End-to-end training demo on a synthetic scene (no datasets offline): a shaded sphere on a
white background, rendered analytically from poses on a camera circle, is learned by a fresh
coarse+fine NeRF pair with the reference's loop (main.py:67-112: random ray batches -> render ->
mse(rgb) + mse(rgb0) -> Adam with exponential lr decay).  Prints PSNR on a held-out view.

    python tools/train_demo.py [--steps 600] [--res 64] [--views 12] [--occupancy 32 --occupancy-warmup 200 --occupancy-refresh 16 [--ray-bounds 256]]

--occupancy RES trains with an occupancy grid of RES^3 cells (occupancy.TrainCull, Renderer.train_occupancy; see train_culled).
--ray-bounds P also clips every ray's near / far to the grid's live span along it, probed at P points (occupancy.RayBounds,
Renderer.ray_bounds), from the moment the grid is filled, and for the test renders.
--live-sampler P places the coarse samples in each ray's live stretches, probed at P points (occupancy.LiveSampler,
Renderer.coarse_sampler; --live-sampler-pad widens every stretch), from the same moment and for the test renders.  Off by default.

    python tools/train_demo.py --refine-poses 3 0.1 [--pose-lr 1e-3] [--freeze-views 1] [--steps 2000] [--out FILE]

--refine-poses ROT_DEG TRANS perturbs every training pose and trains the field and the poses jointly (utils.CapturedJointStep over
utils.LearnedPoses and utils.ImageBankSampler), beside plain training on the perturbed and on the true poses: run_refine_poses.
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("NERF_AMD_QUIET", "1")
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nerf_shared_amd import occupancy, render_utils, synth, utils  # noqa: E402

SPHERE_BOX = [[-1.5, -1.5, -1.5], [1.5, 1.5, 1.5]]          # the unit sphere with room for the dilation


def sphere_image(H, W, K, c2w, dev, radius=1.0, ss=1):
    """Analytic target: Lambert-shaded unit sphere at the origin, white background.  ss > 1: the mean of ss x ss
    sub-pixel samples (an anti-aliased silhouette, as a rendered dataset frame has)."""
    if ss > 1:
        Ks = np.array(K, np.float64).copy()
        Ks[:2, :] *= ss                                      # an ss-times finer pixel grid over the same field of view
        Ks[0, 2] += 0.5 * (ss - 1)
        Ks[1, 2] += 0.5 * (ss - 1)                           # sub-pixel centres symmetric around the coarse pixel centre
        fine = sphere_image(H * ss, W * ss, Ks, c2w, dev, radius, 1)
        return fine.reshape(H, ss, W, ss, 3).mean((1, 3))
    ro, rd = utils.get_rays(H, W, K, torch.from_numpy(c2w))
    rd_n = rd / rd.norm(dim=-1, keepdim=True)
    b = (ro * rd_n).sum(-1)
    disc = b * b - ((ro * ro).sum(-1) - radius * radius)
    hit = disc > 0
    t = -b - torch.sqrt(disc.clamp_min(0))
    n = (ro + rd_n * t[..., None]) / radius
    light = torch.tensor([0.5, 0.4, 0.77], device=dev)
    shade = (n * light).sum(-1).clamp(0.1, 1.0)
    base = 0.5 + 0.5 * n                                    # normal-coloured albedo
    img = torch.where(hit[..., None], base * shade[..., None], torch.ones_like(base))
    return img


def write_blender_scene(root, H, W, poses, images, i_train, i_test):
    """The analytic frames as a NeRF-synthetic scene on disk: transforms_{train,val,test}.json (with the
    reference's near / far keys, load_blender.py:57) + RGBA PNGs (alpha = 0 on the white background)."""
    from nerf_shared_amd import image_io
    angle_x = 2.0 * np.arctan(0.5 * W / synth.lego_intrinsics(H, W)[0, 0])
    for split, ids in (("train", i_train), ("val", [i_test]), ("test", [i_test])):
        os.makedirs(os.path.join(root, split), exist_ok=True)
        meta = {"camera_angle_x": float(angle_x), "near": 2.0, "far": 6.0, "frames": []}
        for k, i in enumerate(ids):
            rgb = images[i].cpu().numpy()
            alpha = (np.abs(rgb - 1.0).max(-1, keepdims=True) > 0).astype(np.float32)       # background is exactly white
            image_io.write_png(os.path.join(root, split, "r_%d.png" % k), utils.to8b(np.concatenate([rgb, alpha], -1)))
            meta["frames"].append({"file_path": "./%s/r_%d" % (split, k), "transform_matrix": poses[i].tolist()})
        with open(os.path.join(root, "transforms_%s.json" % split), "w") as f:
            json.dump(meta, f)


def train_culled(renderer, coarse, fine, opt, H, W, K, chunk, n_rand, next_batch, lr_at, first, steps, box, resolution,
                 warmup=200, refresh=16, calibration_steps=8, slabs=8, margin=1.25, outside="empty", verbose=True,
                 ray_bounds_probes=None, ray_bounds_pad=32, live_sampler_probes=None, live_sampler_pad=1):
    """The training loop with an occupancy grid, steps [first, first + steps):
      1. `warmup` steps through a captured DENSE step (utils.CapturedTrainStep): the field has to mean something first;
      2. OccupancyGrid(box, resolution).fill_from_density([coarse, fine]);
      3. `calibration_steps` eager steps at fraction 1.0 (no saving, but the live counts are exact), then TrainCull.calibrate();
      4. a second captured step, now with Renderer.train_occupancy set: the fractions are frozen in it, the grid is not;
      5. every `refresh` steps one of `slabs` slabs of the grid is re-marked from the models with a new seed
         (refresh_from_density: in place, nothing synchronises), so the grid follows the models; the share of live cells and
         the counts are then read (one synchronisation per refresh, and two soon after a capture) and, when the grid or the
         live share has grown towards the frozen capacities, the fractions are set again and the step is captured again.
    ray_bounds_probes = P: from step 2 on renderer.ray_bounds = RayBounds(grid, P, ray_bounds_pad) (it stays set when this
    returns: the evaluation renders of a model trained on clipped rays clip theirs too).  The pad is wide on purpose -- 32 of
    256 probes of a [2, 6] ray are half a scene unit either side of the live span.  Measured: training at pad 1 or 8
    lost 2.4 dB of test PSNR on the sphere scene, at pad 32 it is level with the dense run (profiles/occupancy_bounds.json);
    rendering a trained model at pad 1 loses nothing.  The cause was not isolated.  We SUPPOSE the compositing's 1e10-long
    last interval (the last sample of a ray should lie in space the model has learnt to be empty) and a grid that follows a
    model which is only ever sampled inside the grid's own span.
    live_sampler_probes = P: from step 2 on renderer.coarse_sampler = LiveSampler(grid, P, live_sampler_pad) as well (it stays
    set when this returns, like the bounds).  Off unless asked for; what training with it was measured to do: DESIGN.md 8e.3.
    next_batch(i) -> (rays [2, n_rand, 3], target [n_rand, 3]); lr_at(i): the learning rate AFTER step i (main.py:108-112).
    Returns (last loss, the TrainCull or None when the run ended inside the warm-up, its stats())."""
    def set_lr(i):
        for g in opt.param_groups:
            g['lr'] = lr_at(i)

    def eager_step(i):
        # In a function of its own: NOTHING with autograd history may outlive it.  A render result left in a local of this
        # loop would keep the parameters' AccumulateGrad nodes -- made on the stream this step ran on -- alive into the
        # construction of the next captured step, whose backward would then hand its gradients to nodes of the default
        # stream from inside a capture.
        rays, target = next_batch(i)
        opt.zero_grad(set_to_none=True)
        rgb, _, _, extras = renderer.render_from_rays(H, W, K, chunk, rays, coarse, fine, retraw=True)
        loss = utils.img2mse(rgb, target)
        if 'rgb0' in extras:
            loss = loss + utils.img2mse(extras['rgb0'], target)
        loss.backward()
        opt.sync_lr()                                        # (after a captured step the update reads the rate on the device)
        opt.step()
        return loss.detach()

    loss, i, last = None, first, first + steps
    renderer.train_occupancy = None
    if ray_bounds_probes:
        occupancy._probes_pad(ray_bounds_probes, ray_bounds_pad)       # a bad pair is refused now, not after the warm-up
        renderer.ray_bounds = None
    if live_sampler_probes:
        occupancy._probes_pad(live_sampler_probes, live_sampler_pad)
        renderer.coarse_sampler = None
    if min(warmup, steps) > 0:
        dense = utils.CapturedTrainStep(renderer, H, W, K, chunk, coarse, fine, opt, n_rand)
        while i < min(first + warmup, last):
            loss = dense(*next_batch(i))
            set_lr(i)
            i += 1
    if i >= last:
        return loss, None, None
    grid = occupancy.OccupancyGrid(box, resolution, outside=outside, device=next(coarse.parameters()).device)
    grid.fill_from_density([coarse, fine])
    cull = occupancy.TrainCull(grid)
    renderer.train_occupancy = cull
    if ray_bounds_probes:
        renderer.ray_bounds = occupancy.RayBounds(grid, ray_bounds_probes, ray_bounds_pad)
    if live_sampler_probes:
        renderer.coarse_sampler = occupancy.LiveSampler(grid, live_sampler_probes, live_sampler_pad)
    for _ in range(min(calibration_steps, last - i)):
        loss = eager_step(i)
        set_lr(i)
        i += 1
    fractions = cull.calibrate(margin)
    if verbose:
        print("occupancy: %.1f %% of the cells live; capacities %.3f (coarse) %.3f (fine) of the samples"
              % (100 * grid.occupied_fraction(), fractions[0], fractions[1]))

    def capture():
        before = cull.totals.clone()
        step = utils.CapturedTrainStep(renderer, H, W, K, chunk, coarse, fine, opt, n_rand)
        cull.totals.copy_(before)                            # (the construction's warm-up steps are not the run's)
        return step

    if i < last:
        cull.stats(reset=True)
        step, seen, captured_at, occupied = capture(), cull.stats(), i, grid.occupied_fraction()
        while i < last:
            loss = step(*next_batch(i))
            set_lr(i)
            i += 1
            refreshed = refresh > 0 and (i - first) % refresh == 0
            grown = 1.0
            if refreshed:
                grid.refresh_from_density([coarse, fine], cells=grid.slab((i - first) // refresh, slabs), seed=i)
                grown = grid.occupied_fraction() / max(occupied, 1e-9)
            if refreshed or i - captured_at in (4, 8):
                # The capacities are frozen in the captured step; the field, and with it the refreshed grid, is not.  Two
                # looks (each reads counts: a synchronisation per refresh, and two soon after a capture): the share of
                # live cells BEFORE the next replay -- a refresh that grew the grid raises the capacities by as much at
                # once --, and the live share of the steps since the last look.  Either one using up a quarter of the
                # margin's headroom sets the fractions again and captures again.
                now = cull.stats()
                if now["coarse"]["total"] == seen["coarse"]["total"]:
                    continue                                 # (no step since the last look: nothing to judge by)
                share = {p: (now[p]["live"] - seen[p]["live"]) / max(now[p]["total"] - seen[p]["total"], 1) for p in cull.PASSES}
                seen = now
                tight = any(share[p] * grown * margin ** 0.75 > getattr(cull, p + "_fraction") for p in cull.PASSES
                            if getattr(cull, p + "_fraction") < 1.0)
                if tight or grown > margin ** 0.25:
                    for p in cull.PASSES:
                        setattr(cull, p + "_fraction", min(1.0, max(margin * share[p] * max(grown, 1.0), 1.0 / n_rand)))
                    step, captured_at, occupied = capture(), i, grid.occupied_fraction()
                    if verbose:
                        print("step %d: capacities now %.3f (coarse) %.3f (fine)" % (i, cull.coarse_fraction, cull.fine_fraction))
    stats = cull.stats()
    for name, s in stats.items():
        if s["overflow"] > 0.01 * max(s["live"], 1):
            print("WARNING: %s pass: %d of %d live samples overflowed the list (treated as empty); raise the margin of calibrate()"
                  % (name, s["overflow"], s["live"]), file=sys.stderr)
    return loss, cull, stats


def run(steps=600, res=64, views=12, n_rand=1024, seed=0, verbose=True, scene_dir=None, multires=10, multires_views=4,
        lrate=5e-4, ss=1, occupancy_res=None, occupancy_warmup=200, occupancy_refresh=16, ray_bounds_probes=None, ray_bounds_pad=32,
        live_sampler_probes=None, live_sampler_pad=1):
    """scene_dir: write the scene to disk in the Blender format first and train from what
    utils.load_datasets reads back (8-bit frames) instead of from the in-memory float images.
    ray_bounds_probes, ray_bounds_pad (with occupancy_res): train_culled's; the test render after training is clipped by the same grid.
    live_sampler_probes, live_sampler_pad (with occupancy_res): train_culled's; the test render uses the same sampler."""
    torch.manual_seed(seed)
    np.random.seed(seed)
    dev = torch.device("cuda:0")
    H = W = res
    K = synth.lego_intrinsics(H, W)
    poses = np.stack([np.concatenate([synth.pose_spherical(th, -30.0 + 20.0 * np.sin(i)), [[0, 0, 0, 1]]], 0)
                      for i, th in enumerate(np.linspace(-180, 180, views + 1)[:-1])], 0).astype(np.float32)
    images = torch.stack([sphere_image(H, W, K, p[:3, :4], dev, ss=ss) for p in poses], 0)
    i_train, i_test = list(range(1, views)), 0
    near, far = 2.0, 6.0
    if scene_dir is not None:
        write_blender_scene(scene_dir, H, W, poses, images, i_train, i_test)
        largs = SimpleNamespace(dataset_type="blender", datadir=scene_dir, half_res=False, testskip=1, white_bkgd=True,
                                render_test=False)
        imgs_np, poses, _, hwf, (i_train, _, i_test_arr), K, bds = utils.load_datasets(largs)
        assert hwf[:2] == [H, W] and abs(hwf[2] - synth.lego_intrinsics(H, W)[0, 0]) < 1e-3 * hwf[2]
        images = torch.from_numpy(np.ascontiguousarray(imgs_np)).float().to(dev)
        i_train, i_test = list(i_train), int(i_test_arr[0])
        near, far = bds["near"], bds["far"]
    args = SimpleNamespace(N_rand=n_rand, no_batching=False, lrate=lrate, lrate_decay=250, netdepth=8, netwidth=256,
                           netdepth_fine=8, netwidth_fine=256, N_importance=128, use_viewdirs=True, multires=multires,
                           multires_views=multires_views, i_embed=0)
    coarse, fine = utils.create_nerf_models(args, dev)
    renderer = render_utils.Renderer(perturb=1.0, N_importance=128, N_samples=64, use_viewdirs=True, white_bkgd=True,
                                     raw_noise_std=0.0, near=near, far=far)
    opt = utils.get_optimizer(coarse, fine, args)
    images, poses_t, rays_rgb, use_batching, N_rand, i_batch = utils.batch_training_data(args, poses, (H, W, K[0][0]), K, images, i_train)

    def test_psnr():
        with torch.no_grad():
            rgb = renderer.render(H, W, K, coarse, fine, chunk=32768, c2w=poses_t[i_test, :3, :4], retraw=False)[0]
            return float(utils.mse2psnr(utils.img2mse(rgb, images[i_test])))

    psnr0 = test_psnr()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cull_stats = None
    if occupancy_res:
        bank = [rays_rgb, i_batch]

        def next_batch(i):
            batch_rays, target, bank[0], bank[1] = utils.sample_random_ray_batch(args, images, poses_t, bank[0], N_rand, use_batching,
                                                                                 bank[1], i_train, (H, W, K[0][0]), K, 0, i)
            return batch_rays, target

        loss, _, cull_stats = train_culled(renderer, coarse, fine, opt, H, W, K, 32768, N_rand, next_batch,
                                           lambda i: args.lrate * (0.1 ** (i / (args.lrate_decay * 1000))), 0, steps, SPHERE_BOX,
                                           int(occupancy_res), occupancy_warmup, occupancy_refresh, verbose=verbose,
                                           ray_bounds_probes=ray_bounds_probes, ray_bounds_pad=ray_bounds_pad,
                                           live_sampler_probes=live_sampler_probes, live_sampler_pad=live_sampler_pad)
        renderer.train_occupancy = None
    for i in range(0 if occupancy_res else steps):          # the dense loop, eager (main.py:77-112)
        batch_rays, target, rays_rgb, i_batch = utils.sample_random_ray_batch(args, images, poses_t, rays_rgb, N_rand, use_batching,
                                                                              i_batch, i_train, (H, W, K[0][0]), K, 0, i)
        opt.zero_grad(set_to_none=True)
        rgb, disp, acc, extras = renderer.render_from_rays(H, W, K, 32768, batch_rays, coarse, fine, retraw=True)
        loss = utils.img2mse(rgb, target) + utils.img2mse(extras['rgb0'], target)
        loss.backward()
        opt.step()
        new_lr = args.lrate * (0.1 ** (i / (args.lrate_decay * 1000)))          # main.py:108-112
        for g in opt.param_groups:
            g['lr'] = new_lr
        if verbose and (i + 1) % 100 == 0:
            print("step %d loss %.5f" % (i + 1, float(loss.detach())))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = {"steps": steps, "rays_per_step": n_rand, "train_s": dt, "steps_per_s": steps / dt,
           "psnr_before": psnr0, "psnr_after": test_psnr(), "final_loss": float(loss.detach())}
    if occupancy_res:
        out["occupancy"] = {"resolution": int(occupancy_res), "warmup": occupancy_warmup, "refresh": occupancy_refresh, "stats": cull_stats}
        if ray_bounds_probes:
            out["occupancy"]["ray_bounds_probes"] = int(ray_bounds_probes)
            out["occupancy"]["ray_bounds_pad"] = int(ray_bounds_pad)
        if live_sampler_probes:
            out["occupancy"]["live_sampler_probes"] = int(live_sampler_probes)
            out["occupancy"]["live_sampler_pad"] = int(live_sampler_pad)
    return out, (coarse, fine, opt, args, renderer, (H, W, K), poses_t, images, i_test)


def rigid_alignment(src, dst):
    """The rigid motion (R [3, 3], t [3]; no scale) that best maps the points src [n, 3] onto dst [n, 3] (Kabsch)."""
    cs, cd = src.mean(0), dst.mean(0)
    U, _, Vt = np.linalg.svd((dst - cd).T @ (src - cs))
    R = U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))]) @ Vt
    return R, cd - R @ cs


def pose_errors(est, true):
    """Rotation (degrees) and translation error of the poses est [n, 4, 4] against true [n, 4, 4], mean over the views, after
    the rigid alignment of the camera centres (a reconstruction is defined up to a rigid motion); also the 4 x 4 alignment."""
    est, true = np.asarray(est, np.float64), np.asarray(true, np.float64)
    R, t = rigid_alignment(est[:, :3, 3], true[:, :3, 3])
    A = np.eye(4)
    A[:3, :3], A[:3, 3] = R, t
    moved = A @ est
    cosines = [(np.trace(m[:3, :3].T @ q[:3, :3]) - 1.0) / 2.0 for m, q in zip(moved, true)]
    rot = float(np.degrees(np.arccos(np.clip(cosines, -1.0, 1.0))).mean())
    return rot, float(np.linalg.norm(moved[:, :3, 3] - true[:, :3, 3], axis=1).mean()), A


def run_refine_poses(rot_deg, trans, steps=2000, res=64, views=12, n_rand=1024, seed=0, lrate=5e-4, pose_lr=1e-3, freeze_views=1,
                     precision="fp32_split", verbose=True):
    """--refine-poses: three legs on the sphere scene with the same seed and steps,
      joint            the training poses perturbed (each view by its own rotation of rot_deg about a random axis and a
                       translation of length trans, utils.perturbed_start_poses' noise), field and poses trained together
                       (utils.CapturedJointStep + utils.ImageBankSampler; the first freeze_views views keep their given pose);
      plain_perturbed  the reference's training on the perturbed poses (utils.CapturedTrainStep);
      plain_true       the same on the true poses.
    Per leg: rotation / translation error of the training poses before and after (pose_errors), and the PSNR of the held-out
    view rendered at its true pose carried into the leg's own frame by the inverse alignment.  Results to report, not gates."""
    from nerf_shared_amd import optim
    dev = torch.device("cuda:0")
    H = W = res
    K = synth.lego_intrinsics(H, W)
    true = np.stack([np.concatenate([synth.pose_spherical(th, -30.0 + 20.0 * np.sin(i)), [[0, 0, 0, 1]]], 0)
                     for i, th in enumerate(np.linspace(-180, 180, views + 1)[:-1])], 0).astype(np.float32)
    images = torch.stack([sphere_image(H, W, K, p[:3, :4], dev) for p in true], 0).contiguous()
    i_train, i_test = list(range(1, views)), 0
    noisy = true.copy()
    for i in i_train:
        noisy[i] = utils.perturbed_start_poses(true[i], 2, rot_deg, trans, seed=1000 * seed + i)[1]
    lr_at = lambda i, base: base * (0.1 ** (i / 250000.0))          # noqa: E731  (main.py:108-112)
    legs = {}
    for leg in ("joint", "plain_perturbed", "plain_true"):
        torch.manual_seed(seed)
        np.random.seed(seed)
        given = true if leg == "plain_true" else noisy
        args = SimpleNamespace(N_rand=n_rand, no_batching=False, lrate=lrate, lrate_decay=250, netdepth=8, netwidth=256,
                               netdepth_fine=8, netwidth_fine=256, N_importance=128, use_viewdirs=True, multires=10,
                               multires_views=4, i_embed=0)
        coarse, fine = utils.create_nerf_models(args, dev)
        coarse.precision = fine.precision = precision
        renderer = render_utils.Renderer(perturb=1.0, N_importance=128, N_samples=64, use_viewdirs=True, white_bkgd=True,
                                         raw_noise_std=0.0, near=2.0, far=6.0)
        field = list(coarse.parameters()) + list(fine.parameters())
        before = pose_errors(given[i_train], true[i_train])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if leg == "joint":
            learned = utils.LearnedPoses(given[i_train], frozen=range(freeze_views)).to(dev)
            opt = optim.Adam([{"params": field, "lr": lrate}, {"params": [learned.twist.xi], "lr": pose_lr}], betas=(0.9, 0.999))
            bank = utils.ImageBankSampler(images[i_train].contiguous(), n_rand, seed=seed)
            step = utils.CapturedJointStep(renderer, H, W, K, 32768, coarse, fine, learned, opt, n_rand, sampler=bank)
            for i in range(steps):
                loss = step()
                opt.param_groups[0]["lr"], opt.param_groups[1]["lr"] = lr_at(i, lrate), lr_at(i, pose_lr)
            final = step.poses.detach().cpu().numpy()
        else:
            opt = optim.Adam(field, lr=lrate, betas=(0.9, 0.999))
            _, poses_t, rays_rgb, use_batching, N_rand, i_batch = utils.batch_training_data(args, given, (H, W, K[0][0]), K, images, i_train)
            step = utils.CapturedTrainStep(renderer, H, W, K, 32768, coarse, fine, opt, n_rand)
            for i in range(steps):
                rays, target, rays_rgb, i_batch = utils.sample_random_ray_batch(args, images, poses_t, rays_rgb, N_rand, use_batching,
                                                                                i_batch, i_train, (H, W, K[0][0]), K, 0, i)
                loss = step(rays, target)
                opt.param_groups[0]["lr"] = lr_at(i, lrate)
            final = given[i_train]
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rot, tr, A = pose_errors(final, true[i_train])
        test_pose = torch.from_numpy((np.linalg.inv(A) @ true[i_test].astype(np.float64)).astype(np.float32))
        with torch.no_grad():
            rgb = renderer.render(H, W, K, coarse, fine, chunk=32768, c2w=test_pose[:3, :4], retraw=False)[0]
            psnr = float(utils.mse2psnr(utils.img2mse(rgb, images[i_test])))
        legs[leg] = {"rot_err_deg_before": before[0], "trans_err_before": before[1], "rot_err_deg_after": rot, "trans_err_after": tr,
                     "test_psnr": psnr, "final_loss": float(loss), "train_s": dt}
        if verbose:
            print(leg, json.dumps(legs[leg]))
        del step, opt, coarse, fine
    return {"scene": "sphere", "res": res, "views": views, "train_views": len(i_train), "steps": steps, "rays_per_step": n_rand,
            "seed": seed, "precision": precision, "perturbation": {"rot_deg": rot_deg, "trans": trans}, "lrate": lrate,
            "pose_lr": pose_lr, "freeze_views": freeze_views, "legs": legs}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--refine-poses", type=float, nargs=2, default=None, metavar=("ROT_DEG", "TRANS"),
                    help="perturb every training pose by this rotation and translation and train field and poses jointly; runs the "
                    "three legs of run_refine_poses and prints their table")
    ap.add_argument("--pose-lr", type=float, default=1e-3, help="--refine-poses: the learning rate of the pose twists")
    ap.add_argument("--freeze-views", type=int, default=1, metavar="N", help="--refine-poses: the first N training views keep their pose (gauge)")
    ap.add_argument("--precision", choices=["bf16", "fp32_split", "fp32"], default="fp32_split", help="--refine-poses: the fields' arithmetic")
    ap.add_argument("--out", default=None, help="--refine-poses: write the result here as JSON")
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--scene-dir", default=None, help="write the scene in the Blender format here and train from disk")
    ap.add_argument("--multires", type=int, default=10)
    ap.add_argument("--multires-views", type=int, default=4)
    ap.add_argument("--n-rand", type=int, default=1024)
    ap.add_argument("--lrate", type=float, default=5e-4)
    ap.add_argument("--ss", type=int, default=1, help="ss x ss sub-pixel samples per ground-truth pixel")
    ap.add_argument("--quiet", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--occupancy", type=int, default=0, metavar="RES", help="train with an occupancy grid of RES^3 cells (0: dense)")
    ap.add_argument("--occupancy-warmup", type=int, default=200, metavar="N", help="dense steps before the grid is filled")
    ap.add_argument("--occupancy-refresh", type=int, default=16, metavar="K", help="re-mark a slab of the grid every K steps (0: never)")
    ap.add_argument("--ray-bounds", type=int, default=0, metavar="P", help="with --occupancy: clip each ray's near / far to the grid's "
                    "live span, probed at P points (a power of two in 64..4096; 0: off)")
    ap.add_argument("--ray-bounds-pad", type=int, default=32, metavar="N", help="probe spacings the span is widened by while training")
    ap.add_argument("--live-sampler", type=int, default=0, metavar="P", help="with --occupancy: place the coarse samples in each ray's "
                    "live stretches, probed at P points (a power of two in 64..4096; 0: off)")
    ap.add_argument("--live-sampler-pad", type=int, default=1, metavar="N", help="probes every live stretch is widened by, either way")
    a = ap.parse_args()
    if a.refine_poses is not None:
        result = run_refine_poses(a.refine_poses[0], a.refine_poses[1], steps=a.steps, res=a.res, views=a.views, n_rand=a.n_rand, seed=a.seed,
                                  lrate=a.lrate, pose_lr=a.pose_lr, freeze_views=a.freeze_views, precision=a.precision, verbose=not a.quiet)
        print(json.dumps(result, indent=1))
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(result, indent=1) + "\n")
        sys.exit(0)
    print(json.dumps(run(a.steps, a.res, a.views, n_rand=a.n_rand, seed=a.seed, scene_dir=a.scene_dir, multires=a.multires,
                         multires_views=a.multires_views, lrate=a.lrate, ss=a.ss, verbose=not a.quiet, occupancy_res=a.occupancy or None,
                         occupancy_warmup=a.occupancy_warmup, occupancy_refresh=a.occupancy_refresh,
                         ray_bounds_probes=a.ray_bounds or None, ray_bounds_pad=a.ray_bounds_pad,
                         live_sampler_probes=a.live_sampler or None, live_sampler_pad=a.live_sampler_pad)[0]))
