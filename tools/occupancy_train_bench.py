#!/usr/bin/env python3
"""What the occupancy grid buys a TRAINING step and a POSE step (occupancy.TrainCull, Renderer.train_occupancy): trains the sphere
scene of tools/train_demo.py (1500 steps), fills the grid of profiles/occupancy_render.json (128^3, outside 'empty') and times
three captured steps that alternate in one process -- no train_occupancy; an all-live grid at fraction 1.0 (what the new
launches cost); the filled grid at calibrated fractions -- for utils.CapturedTrainStep (1024 rays, 64 + 128 samples) and
utils.CapturedPoseStep (512 pixels), in bf16 and fp32_split; device events around each replay, median of --reps after --warmup.
--learning adds what tests/test_gpu_train_cull.py's learning test needs: the test PSNR of 600 dense steps of the sphere scene
for three seeds (their spread is the test's margin) and of the culled run of seed 0.  Writes profiles/occupancy_train.json.

    python tools/occupancy_train_bench.py [--steps 1500] [--reps 9] [--learning] [--out profiles/occupancy_train.json]

The dense leg is the parent's step launch for launch; compare it with tools/train_bench.py --graph of the parent commit on
the same machine, alternating, each run under its own time limit:

    timeout -k 10 300 python tools/train_bench.py --graph && timeout -k 10 300 python <parent>/tools/train_bench.py --graph && ...
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
os.environ.setdefault("NERF_AMD_QUIET", "1")
import numpy as np  # noqa: E402
import torch  # noqa: E402

import train_demo  # noqa: E402
from nerf_shared_amd import occupancy, optim, render_utils, synth, utils  # noqa: E402
from occupancy_bench import BOX, spread, timed  # noqa: E402

CFG = dict(N_importance=128, N_samples=64, use_viewdirs=True, white_bkgd=True, raw_noise_std=0.0, near=2.0, far=6.0)
LEGS = ("dense", "all_live", "culled")


def fractions_of(cull):
    return {"coarse": cull.coarse_fraction, "fine": cull.fine_fraction}


def alternate(steps, calls, culls, warmup, reps):
    """steps / calls: per leg, the captured step and the arguments of one replay.  Returns per leg the replay times and, for
    the legs that cull, the counts of the timed replays."""
    times = {k: [] for k in steps}
    for i in range(warmup + reps):
        if i == warmup:
            for c in culls.values():
                c.stats(reset=True)
        for name, step in steps.items():                 # alternating: every leg sees the same clocks and the same neighbours
            ms, _ = timed(lambda: step(*calls[name]))
            if i >= warmup:
                times[name].append(ms)
    return {k: spread(v) for k, v in times.items()}, {k: c.stats() for k, c in culls.items()}


def calibrated(renderer, grid, eager_step, n=8, margin=1.25):
    """A TrainCull on `grid`, its fractions set from n eager steps at fraction 1.0."""
    cull = occupancy.TrainCull(grid)
    renderer.train_occupancy = cull
    for _ in range(n):
        eager_step(renderer)
    cull.calibrate(margin)
    return cull


def bench_train(models, grid, all_live, dev, rays, warmup, reps):
    H = W = 400
    K = synth.lego_intrinsics(H, W)
    rng = np.random.default_rng(0)
    pose = synth.pose_spherical(30.0, -30.0)                                   # a view of the sphere from the training circle's radius
    ro, rd = synth.rays_np(H, W, K, pose, rng.choice(H * W, size=rays, replace=False))
    batch = torch.from_numpy(np.stack([ro, rd], 0)).to(dev)
    target = torch.rand(rays, 3, device=dev)
    params = list(models[0].parameters()) + list(models[1].parameters())
    snapshot = [p.detach().clone() for p in params]

    def eager_step(r):
        for p in params:
            p.grad = None
        rgb, _, _, ex = r.render_from_rays(H, W, K, 32768, batch, models[0], models[1], retraw=True)
        (utils.img2mse(rgb, target) + utils.img2mse(ex["rgb0"], target)).backward()

    steps, culls = {}, {}
    for name in LEGS:
        r = render_utils.Renderer(perturb=1.0, **CFG)
        if name == "all_live":
            culls[name] = r.train_occupancy = occupancy.TrainCull(all_live)
        elif name == "culled":
            culls[name] = calibrated(r, grid, eager_step)
        steps[name] = utils.CapturedTrainStep(r, H, W, K, 32768, models[0], models[1], optim.Adam(params, lr=5e-4, betas=(0.9, 0.999)), rays)
    times, stats = alternate(steps, {k: (batch, target) for k in LEGS}, culls, warmup, reps)
    with torch.no_grad():                                                      # the replays trained on noise: put the scene back
        for p, p0 in zip(params, snapshot):
            p.copy_(p0)
    for m in models:
        m.weights_changed()
    return {"rays": rays, "ms_per_replay": times, "fractions": {k: fractions_of(c) for k, c in culls.items()}, "counts": stats,
            "culled_over_dense": times["culled"]["median_ms"] / times["dense"]["median_ms"],
            "all_live_over_dense": times["all_live"]["median_ms"] / times["dense"]["median_ms"]}


def bench_pose(models, grid, all_live, dev, pixels, pose, warmup, reps):
    H = W = 64
    K = synth.lego_intrinsics(H, W)
    for m in models:
        m.requires_grad_(False)
    r0 = render_utils.Renderer(perturb=0.0, **CFG)
    with torch.no_grad():
        image = r0.render(H, W, K, models[0], models[1], chunk=32768, c2w=pose[:3, :4], retraw=False)[0]
    rng = np.random.default_rng(1)
    idx = rng.choice(H * W, size=pixels, replace=False)
    pix = torch.from_numpy(np.stack([idx % W, idx // W], -1).astype(np.int32)).to(dev)
    target = image[pix[:, 1].long(), pix[:, 0].long()].contiguous()
    start = torch.cat([pose[:3, :4], torch.tensor([[0, 0, 0, 1.0]], device=dev)], 0)

    def fresh():
        cam = utils.CameraTransf()
        with torch.no_grad():
            for p, v in zip(cam.parameters(), ([0.30, -0.25, 0.35], [0.30, -0.20, 0.25], 0.05)):
                p.copy_(torch.tensor(v))
        return cam.to(dev)

    probe = fresh()

    def eager_step(r):
        for p in probe.parameters():
            p.grad = None
        ro, rd = utils.get_rays_at(H, W, K, probe(start), pix)
        rgb = r.render_from_rays(H, W, K, 32768, torch.stack([ro, rd], 0), models[0], models[1], retraw=True)[0]
        utils.img2mse(rgb, target).backward()

    steps, culls = {}, {}
    for name in LEGS:
        r = render_utils.Renderer(perturb=0.0, **CFG)
        if name == "all_live":
            culls[name] = r.train_occupancy = occupancy.TrainCull(all_live)
        elif name == "culled":
            culls[name] = calibrated(r, grid, eager_step)
        cam = fresh()
        steps[name] = utils.CapturedPoseStep(r, H, W, K, 32768, models[0], models[1], cam, start, optim.Adam(cam.parameters(), lr=1e-4), pixels)
    times, stats = alternate(steps, {k: (pix, target) for k in LEGS}, culls, warmup, reps)
    for m in models:
        m.requires_grad_(True)
    return {"pixels": pixels, "ms_per_replay": times, "fractions": {k: fractions_of(c) for k, c in culls.items()}, "counts": stats,
            "culled_over_dense": times["culled"]["median_ms"] / times["dense"]["median_ms"],
            "all_live_over_dense": times["all_live"]["median_ms"] / times["dense"]["median_ms"]}


def learning(steps=600):
    """The numbers of the learning test: 600 dense steps for three seeds (the spread of their test PSNR is the margin) and the
    culled run of seed 0 with the test's flags."""
    dense = [train_demo.run(steps=steps, seed=s, verbose=False)[0]["psnr_after"] for s in (0, 1, 2)]
    culled = train_demo.run(steps=steps, seed=0, verbose=False, occupancy_res=32, occupancy_warmup=200, occupancy_refresh=16)[0]
    return {"steps": steps, "flags": "--occupancy 32 --occupancy-warmup 200 --occupancy-refresh 16",
            "dense_psnr_by_seed": {str(s): v for s, v in zip((0, 1, 2), dense)}, "dense_psnr_spread": max(dense) - min(dense),
            "culled_psnr_seed0": culled["psnr_after"], "culled_stats": culled["occupancy"]["stats"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--pixels", type=int, default=512)
    ap.add_argument("--learning", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "occupancy_train.json"))
    a = ap.parse_args()

    train, (coarse, fine, _, _, _, _, poses_t, _, i_test) = train_demo.run(steps=a.steps, verbose=False)
    dev = torch.device("cuda:0")
    models = (coarse, fine)
    grid = occupancy.OccupancyGrid(BOX, a.grid, outside="empty", device=dev)
    grid.fill_from_density([coarse, fine])
    all_live = occupancy.OccupancyGrid(BOX, a.grid, outside="live", device=dev)
    out = {"workload": "sphere scene of tools/train_demo.py, %d steps; captured steps, 64 + 128 samples; ms per replay between device "
                       "events, three legs alternating, median of %d after %d warm-ups" % (a.steps, a.reps, a.warmup),
           "train": train,
           "grid": {"resolution": a.grid, "box": BOX, "outside": "empty", "samples_per_cell": 4, "dilate": 1,
                    "occupied_fraction": grid.occupied_fraction()},
           "train_step": {}, "pose_step": {}}
    for precision in ("bf16", "fp32_split"):
        for m in models:
            m.precision = precision
        out["train_step"][precision] = bench_train(models, grid, all_live, dev, a.rays, a.warmup, a.reps)
        out["pose_step"][precision] = bench_pose(models, grid, all_live, dev, a.pixels, poses_t[i_test], a.warmup, a.reps)
    def write():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    write()
    if a.learning:
        out["learning"] = learning()
        write()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
